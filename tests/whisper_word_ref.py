"""NumPy / torch restatement of Whisper's token timestamps and the fixture of tests/golden/whisper_word.npz.

Restated from $TF/models/whisper/generation_whisper.py:
  * `dtw`            - `_dynamic_time_warping`: the same table in fp32, the same strict comparisons in the same order, the
    same backtrace; swept by anti-diagonals with NumPy instead of cell by cell (cells with i + j constant are independent);
  * `median_filter`  - `_median_filter` (reflect padding, torch.sort: NaN last);
  * `cost_from_weights`, `cost_from_qk` - the weights' way to the DTW in `_extract_token_timestamps`: crop to F_b, standardise
    over the tokens (population standard deviation), median filter along time, mean over the heads, negate;
  * `jump_frames`, `token_times` - the first path step of every text index, and a row's times.

The fixture is that of tests/whisper_ts_ref.py (seeded model, seeded audio) with ALIGNMENT_HEADS over both decoder layers;
the short clips' valid frames are their true lengths, so every clip has its own F_b.  tools/gen_whisper_word_goldens.py
records transformers' own results; tests/test_whisper_word_cpu.py holds this file against them."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch

import whisper_ts_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "whisper_word.npz"
ALIGNMENT_HEADS = [(0, 1), (1, 0), (1, 3), (0, 2)]
FILTER_WIDTH = 7
SHORT_NUM_FRAMES = [int(round(s * 100)) for s in R.SHORT_SECONDS]  # 400, 1150, 2700 log-mel frames
TIME_PRECISION = 0.02


# ---- dynamic time warping ----------------------------------------------------------------------------------------------
def dtw(matrix):
    """matrix [Lw, F] -> (text indices, time indices) of the path, as `_dynamic_time_warping(matrix)`."""
    m = np.asarray(matrix, dtype=np.float32)
    N, M = m.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = -np.ones((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    with np.errstate(invalid="ignore"):
        for k in range(2, N + M + 1):
            i = np.arange(max(1, k - M), min(N, k - 1) + 1)
            j = k - i
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            t0 = (c0 < c1) & (c0 < c2)
            t1 = ~t0 & (c1 < c0) & (c1 < c2)
            c = np.where(t0, c0, np.where(t1, c1, c2))
            cost[i, j] = m[i - 1, j - 1] + c
            trace[i, j] = np.where(t0, 0, np.where(t1, 1, 2))
    i, j = N, M
    trace[0, :] = 2
    trace[:, 0] = 1
    text, time = [], []
    while i > 0 or j > 0:
        text.append(i - 1)
        time.append(j - 1)
        t = trace[i, j]
        if t == 0:
            i, j = i - 1, j - 1
        elif t == 1:
            i -= 1
        elif t == 2:
            j -= 1
        else:
            raise RuntimeError(f"unexpected trace[{i}, {j}]")
    return np.array(text, dtype=np.int64)[::-1], np.array(time, dtype=np.int64)[::-1]


def dtw_branches(matrix):
    """How often each clause of the rule decides a cell: diagonal strictly lowest; upper strictly lowest; left strictly
    lowest; and the ties that fall to the left cell (diag == up lowest, diag == left lowest, up == left lowest)."""
    m = np.asarray(matrix, dtype=np.float32)
    N, M = m.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    cost[0, 0] = 0
    seen = dict(diag=0, up=0, left=0, tie_diag_up=0, tie_diag_left=0, tie_up_left=0)
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        t0 = (c0 < c1) & (c0 < c2)
        t1 = ~t0 & (c1 < c0) & (c1 < c2)
        fin = np.isfinite(c0) & np.isfinite(c1) & np.isfinite(c2)
        seen["diag"] += int(t0.sum())
        seen["up"] += int(t1.sum())
        seen["left"] += int((fin & (c2 < c0) & (c2 < c1)).sum())
        seen["tie_diag_up"] += int((fin & (c0 == c1) & (c0 < c2)).sum())
        seen["tie_diag_left"] += int((fin & (c0 == c2) & (c0 < c1)).sum())
        seen["tie_up_left"] += int((fin & (c1 == c2) & (c1 < c0)).sum())
        cost[i, j] = m[i - 1, j - 1] + np.where(t0, c0, np.where(t1, c1, c2))
    return seen


def path_cost(matrix, text, time) -> float:
    """The sum of the matrix along a path, in float64."""
    return float(np.asarray(matrix, dtype=np.float64)[np.asarray(text), np.asarray(time)].sum())


def jump_frames(text, time):
    """The time index at the first path step of every text index (`time_indices[jumps]`)."""
    text, time = np.asarray(text), np.asarray(time)
    jumps = np.pad(np.diff(text), (1, 0), constant_values=1).astype(bool)
    return time[jumps]


def token_times(jump, prefix_len, total_len):
    """One row: P zeros, the jump times, the last one again (float32, as the float32 `timestamps` tensor stores them)."""
    jt = np.asarray(jump, dtype=np.int64) * TIME_PRECISION
    row = np.zeros(total_len, dtype=np.float32)
    if len(jt):
        row[prefix_len:prefix_len + len(jt)] = jt
        row[prefix_len + len(jt)] = jt[-1]
    return row


# ---- the cost matrix -------------------------------------------------------------------------------------------------------
def median_filter(x: torch.Tensor, width: int) -> torch.Tensor:
    if width <= 0 or width % 2 != 1:
        raise ValueError("`filter_width` should be an odd number")
    pad = width // 2
    if x.shape[-1] <= pad:
        return x
    x = torch.nn.functional.pad(x, (pad, pad, 0, 0), mode="reflect")
    return x.unfold(-1, width, 1).sort()[0][..., pad]


def frames_of(num_frames, B, Te=1500):
    if num_frames is None:
        return [Te] * B
    return [max(1, min(Te, int(n) // 2)) for n in num_frames]


def cost_from_weights(weights: torch.Tensor, F: int, width: int = FILTER_WIDTH) -> torch.Tensor:
    """weights [A, Lw, Te] of one clip (any float dtype) -> the DTW's matrix [Lw, F] in that dtype."""
    m = weights[..., :F]
    std = torch.std(m, dim=-2, keepdim=True, unbiased=False)
    mean = torch.mean(m, dim=-2, keepdim=True)
    m = median_filter((m - mean) / std, width)
    return -m.mean(dim=0)


def cost_from_qk(q: torch.Tensor, k: torch.Tensor, F: int, scale: float, width: int = FILTER_WIDTH, dtype=torch.float32):
    """q [A, Lw, hd], k [A, Te, hd] of one clip (the bf16 values, as floats) -> [Lw, F]: the formula of
    ca_whisper_align_cost evaluated by torch in `dtype`."""
    q, k = q.to(dtype), k.to(dtype)
    w = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
    return cost_from_weights(w, F, width)


def oracle_cross_weights(ids: torch.Tensor, enc: torch.Tensor, P: dict, c, heads) -> torch.Tensor:
    """fp32 oracle: the cross-attention probabilities of the alignment heads at every input position of ids [B, L]
    -> [B, A, L, Te] (the layers of oracle.whisper_ref.decoder, with the probabilities of `_attn` kept)."""
    import torch.nn.functional as Fn

    from oracle import whisper_ref as w

    B, L = ids.shape
    H = c.decoder_attention_heads
    hd = c.d_model // H
    out = [None] * len(heads)
    with torch.no_grad():
        h = P["model.decoder.embed_tokens.weight"][ids] + P["model.decoder.embed_positions.weight"][:L]
        for l in range(c.decoder_layers):
            p = f"model.decoder.layers.{l}."
            x = w._ln(h, P, p + "self_attn_layer_norm", c.layer_norm_eps)
            h = h + w._attn(x, x, P, p + "self_attn.", H, causal=True)
            x = w._ln(h, P, p + "encoder_attn_layer_norm", c.layer_norm_eps)
            q = (Fn.linear(x, P[p + "encoder_attn.q_proj.weight"], P[p + "encoder_attn.q_proj.bias"]) * hd ** -0.5)
            q = q.view(B, L, H, hd).transpose(1, 2)
            k = Fn.linear(enc, P[p + "encoder_attn.k_proj.weight"]).view(B, -1, H, hd).transpose(1, 2)
            pr = torch.softmax(q @ k.transpose(-1, -2), -1)
            for a, (la, hh) in enumerate(heads):
                if la == l:
                    out[a] = pr[:, hh]
            h = h + w._attn(x, enc, P, p + "encoder_attn.", H)
            y = w._ln(h, P, p + "final_layer_norm", c.layer_norm_eps)
            y = Fn.linear(Fn.gelu(Fn.linear(y, P[p + "fc1.weight"], P[p + "fc1.bias"])), P[p + "fc2.weight"], P[p + "fc2.bias"])
            h = h + y
    return torch.stack(out, 1)


def oracle_costs(ids, feats, P, c, num_frames, heads=ALIGNMENT_HEADS, prefix_len=len(R.PREFIX), width=FILTER_WIDTH):
    """-> per clip the fp32 oracle's DTW matrix [Lw, F_b] for id rows [B, Ltot]."""
    from oracle import whisper_ref as w

    ids = torch.as_tensor(ids)
    with torch.no_grad():
        enc = w.encoder(feats, P, c)
    wts = oracle_cross_weights(ids[:, :-1], enc, P, c, heads)[:, :, prefix_len:]
    return [cost_from_weights(wts[b], F, width).numpy() for b, F in enumerate(frames_of(num_frames, ids.shape[0]))]


# ---- synthetic DTW cases ---------------------------------------------------------------------------------------------------
# name -> (Lw, F, seed, quantum): uniform noise in [-2, 2); quantum > 0 rounds to its multiples (exact ties)
DTW_CASES = {"l1_f5": (1, 5, 11, 0.0), "l3_f2": (3, 2, 12, 0.0), "l9_f4": (9, 4, 13, 0.0), "l65_f130": (65, 130, 14, 0.0),
             "l447_f1500": (447, 1500, 15, 0.0), "mix_f1500": (40, 1500, 16, 0.0), "mix_f37": (40, 37, 17, 0.0),
             "mix_f4": (40, 4, 18, 0.0), "ties": (33, 70, 19, 0.25), "ties_small": (12, 9, 20, 0.25)}
DTW_MIXED = ("mix_f1500", "mix_f37", "mix_f4")


def dtw_case(name):
    Lw, F, seed, quantum = DTW_CASES[name]
    m = np.random.RandomState(seed).uniform(-2.0, 2.0, size=(Lw, F)).astype(np.float32)
    if quantum:
        m = (np.round(m / quantum) * quantum).astype(np.float32)
    return m


# ---- word grouping: a stand-in tokenizer whose decode joins strings from a table -------------------------------------------
WORD_TABLE = [" hel", "lo", " wor", "ld", ",", ".", " (", "x", ")", "!", " -", "dash", " two", " \"", "q", "\"", "'", "s", " a",
              "?", " ", "é", " 12", "3", ":", " end"]
WORD_EOS = 40          # ids >= WORD_EOS are "special" for _split_tokens_on_spaces
WORD_TIMESTAMP_BEGIN = 50
WORD_CASES = [[0, 1, 2, 3, 4, 12, 5], [6, 7, 8, 9], [10, 11, 12], [13, 14, 15, 16, 17], [18, 19, 18, 20, 21], [22, 23, 24, 25],
              [1, 3, 5, 5], [4], [], [0, 41, 1, 2], [10, 6, 0, 8, 5, 9]]
# (ids with timestamp tokens, a time per id): one window; two segments; a second window whose timestamps restart
ASR_CASES = [
    ([50, 0, 1, 2, 3, 60, 60, 12, 5, 75, 75], [0.0, 0.1, 0.32, 0.5, 0.74, 0.9, 0.9, 1.2, 1.31, 1.5, 1.5]),
    ([50, 18, 19, 90], [0.0, 0.2, 0.46, 0.46]),
    ([50, 0, 1, 70, 70, 2, 3, 4, 95, 95, 52, 12, 5, 64, 64],
     [0.0, 0.08, 0.3, 0.4, 0.4, 0.55, 0.81, 0.93, 1.9, 1.9, 1.9, 2.04, 2.3, 2.56, 2.56]),
    ([50, 6, 7, 8, 9], [0.0, 0.11, 0.27, 0.33, 0.335]),
]


def word_decode(tokens) -> str:
    return "".join(WORD_TABLE[t] if t < len(WORD_TABLE) else f"<|{t}|>" for t in tokens)


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    assert json.loads(str(z["recipe"])) == R.RECIPE, "tests/golden/whisper_word.npz was written with another recipe"
    assert json.loads(str(z["alignment_heads"])) == [list(h) for h in ALIGNMENT_HEADS]
    return z
