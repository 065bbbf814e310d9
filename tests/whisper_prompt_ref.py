"""The fixture of tests/golden/whisper_prompt.npz and an fp32 restatement of Whisper's decoder under a
decoder_attention_mask.

The model, its recipe and its audio are those of tests/whisper_ts_ref.py (a seeded random-init model) with
MAX_TARGET_POSITIONS target positions instead of 64: previous text is cut at CUT_OFF tokens, which some rows reach while
others stay below it with different amounts of text.  The recordings of SECONDS are decoded as one long-form batch.
tools/gen_whisper_prompt_goldens.py records what transformers' long-form `generate` does with them under
`condition_on_prev_tokens`, `prompt_ids` and `prompt_condition_type`, with and without temperature fallback: per round
the windows, the decoder inputs and their mask, the generated ids and (for the rounds listed there) the logits of the
first free position; at the end the segments.

`masked_decoder` is oracle.whisper_ref.decoder with the key mask transformers builds from the decoder_attention_mask
(`create_causal_mask`: causal AND key-is-not-padding) and transformers' position ids: `WhisperDecoder.forward` embeds
arange(P) over the PADDED row, so the padding counts as positions and every row of a step stands at one position.
positions="mask" gives the other reading (positions counted from the first valid token), which the goldens tool holds
against the recorded logits to show that it is not what transformers computes."""
from __future__ import annotations

import json
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

import whisper_ts_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "whisper_prompt.npz"

PREV_SOT = 55                       # <|startofprev|> of the fixture: a special id the ts fixture leaves unused
PROMPT = (PREV_SOT, 7, 21, 33, 4)   # what get_prompt_ids would return: <|startofprev|>, then text
SECONDS = (70.0, 95.0, 41.0)
SEEDS = (800, 801, 812)
MAX_TARGET_POSITIONS = 128
CONFIG = dict(R.CONFIG, max_target_positions=MAX_TARGET_POSITIONS)
CUT_OFF = MAX_TARGET_POSITIONS // 2 - 1
FALLBACK_TEMPERATURES = (0.0, 0.6)
# name -> the arguments of transformers' generate that the run adds
RUNS = {
    "prev": dict(condition_on_prev_tokens=True),
    "first": dict(condition_on_prev_tokens=True, prompt_ids=PROMPT, prompt_condition_type="first-segment"),
    "all": dict(condition_on_prev_tokens=True, prompt_ids=PROMPT, prompt_condition_type="all-segments"),
    "prompt": dict(condition_on_prev_tokens=False, prompt_ids=PROMPT),
    "fallback": dict(condition_on_prev_tokens=True, temperature=FALLBACK_TEMPERATURES),  # + logprob_threshold (recorded)
}
BRANCHES = ("first_window_without_prev", "different_padding_in_a_batch", "cut_at_cut_off", "double_timestamp_ending",
            "first_segment_prompt", "all_segments_prompt", "batch_shrinks", "unconditioned_after_hot_fallback")


def fixture_config():
    from oracle import whisper_ref as w

    return w.WhisperConfig(**CONFIG)


def fixture_params():
    """whisper_ts_ref.fixture_params (its RECIPE, its arithmetic) for CONFIG."""
    from oracle import whisper_ref as w

    r, c = R.RECIPE, fixture_config()
    P = w.synth_params(c)
    g = torch.Generator().manual_seed(int(r["seed"]))
    gdir = torch.randn(c.d_model, generator=g)
    gdir = gdir / gdir.norm()
    delta = r["delta0"] + r["delta1"] * torch.randn(R.N_TS, generator=g)
    P["model.decoder.layer_norm.bias"] = P["model.decoder.layer_norm.bias"] + r["gamma"] * gdir
    E = P["model.decoder.embed_tokens.weight"].clone()
    E[R.TIMESTAMP_BEGIN:] = r["scale"] * E[R.TIMESTAMP_BEGIN:] - delta[:, None] * gdir[None, :]
    E[R.EOS] = E[R.EOS] + r["eps"] * gdir
    P["model.decoder.embed_tokens.weight"] = E
    return P


def waves():
    return [R.fixture_wave(s, seed) for s, seed in zip(SECONDS, SEEDS)]


def features() -> list:
    """Whole-recording log-mel [80, frames] per recording."""
    from oracle import whisper_ref as w

    return [torch.from_numpy(w.log_mel(a)) for a in waves()]


def window_batch(mels, batch) -> torch.Tensor:
    """[(clip, seek)] -> the windows' features [n, 80, 3000]."""
    return torch.stack([R.window_features(mels[c], s) for c, s in batch])


def policy_of(run: str):
    from coral_amd.longform_whisper import PromptPolicy

    kw = RUNS[run]
    return PromptPolicy(prompt_ids=kw.get("prompt_ids"), prompt_condition_type=kw.get("prompt_condition_type"),
                        condition_on_prev_tokens=bool(kw.get("condition_on_prev_tokens")), prev_sot_token_id=PREV_SOT)


def load_golden():
    z = np.load(GOLDEN, allow_pickle=False)
    assert json.loads(str(z["recipe"])) == R.RECIPE, "tests/golden/whisper_prompt.npz was written with another recipe"
    return z


def rounds_of(z, run: str) -> list:
    """The recorded attempts of a run, in order: dict(round, attempt, T, batch [(clip, seek)], rows, start, mask, ids
    (generated, with EOS, padding stripped), avg_logprob, n_scored, needs, logits or None)."""
    meta = json.loads(str(z[f"{run}_meta"]))
    out = []
    r0 = lpos = 0
    with_logits = set(z[f"{run}_logits_row"].tolist())
    for k, m in enumerate(meta):
        n = len(m["batch"])
        sl = slice(r0, r0 + n)
        P = int(m["P"])
        rows = z[f"{run}_dec_ids"][sl, :P]
        mask = rows != R.EOS
        gl = z[f"{run}_gen_len"][sl]
        gen = [z[f"{run}_gen_ids"][r0 + i, :int(gl[i])].tolist() for i in range(n)]
        lg = None
        if r0 in with_logits:
            lg = z[f"{run}_logits"][lpos:lpos + n]
            lpos += n
        out.append(dict(round=m["round"], attempt=m["attempt"], T=m["T"], batch=[tuple(b) for b in m["batch"]], rows=rows,
                        start=(~mask).sum(1), mask=mask, masked=m["masked"], ids=gen, max_length=m["max_length"],
                        avg_logprob=z[f"{run}_avg_logprob"][sl], n_scored=z[f"{run}_n_scored"][sl],
                        needs=z[f"{run}_needs"][sl], logits=lg))
        r0 += n
    return out


def masked_decoder(input_ids, mask, enc, P, c, positions: str = "padded"):
    """input_ids i64 [B, L], mask bool [B, L] (False = padding, a left run), enc [B, 1500, d] -> fp32 logits [B, L, V].
    The rows of padded positions are whatever falls out (transformers' too): nothing valid attends to them."""
    from oracle import whisper_ref as w

    B, L = input_ids.shape
    mask = torch.as_tensor(mask, dtype=torch.bool)
    if positions == "padded":
        pos = torch.arange(L)[None, :].expand(B, L)
    else:
        pos = (mask.long().cumsum(1) - 1).clamp(min=0)
    h = P["model.decoder.embed_tokens.weight"][input_ids] + P["model.decoder.embed_positions.weight"][pos]
    H = c.decoder_attention_heads
    hd = c.d_model // H
    allowed = torch.ones(L, L, dtype=torch.bool).tril()[None, None] & mask[:, None, None, :]
    # (a padded query row has no allowed key; transformers adds finfo.min instead of -inf, so such a row is a uniform
    # average - unused.  Here it attends to itself, which keeps the softmax finite.)
    allowed = allowed | (torch.eye(L, dtype=torch.bool)[None, None] & ~mask[:, None, :, None])
    for l in range(c.decoder_layers):
        p = f"model.decoder.layers.{l}."
        x = w._ln(h, P, p + "self_attn_layer_norm", c.layer_norm_eps)
        a = p + "self_attn."
        q = (F.linear(x, P[a + "q_proj.weight"], P[a + "q_proj.bias"]) * hd ** -0.5).view(B, L, H, hd).transpose(1, 2)
        k = F.linear(x, P[a + "k_proj.weight"]).view(B, L, H, hd).transpose(1, 2)
        v = F.linear(x, P[a + "v_proj.weight"], P[a + "v_proj.bias"]).view(B, L, H, hd).transpose(1, 2)
        s = (q @ k.transpose(-1, -2)).masked_fill(~allowed, float("-inf"))
        o = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, L, c.d_model)
        h = h + F.linear(o, P[a + "out_proj.weight"], P[a + "out_proj.bias"])
        x = w._ln(h, P, p + "encoder_attn_layer_norm", c.layer_norm_eps)
        h = h + w._attn(x, enc, P, p + "encoder_attn.", H)
        y = w._ln(h, P, p + "final_layer_norm", c.layer_norm_eps)
        h = h + F.linear(F.gelu(F.linear(y, P[p + "fc1.weight"], P[p + "fc1.bias"])), P[p + "fc2.weight"], P[p + "fc2.bias"])
    h = w._ln(h, P, "model.decoder.layer_norm", c.layer_norm_eps)
    return F.linear(h, P["model.decoder.embed_tokens.weight"])


def greedy_rows(rows, mask, enc, P, c, max_length: int):
    """Greedy decoding of left-padded rows under [begin-suppress, timestamp rules beginning at P] with masked_decoder,
    one teacher-forced pass per token (tiny model).  -> generated id lists (EOS included)."""
    ids = torch.as_tensor(rows, dtype=torch.int64)
    mask = torch.as_tensor(mask, dtype=torch.bool)
    B, P0 = ids.shape
    gen = [[] for _ in range(B)]
    live = list(range(B))
    while live and ids.shape[1] < max_length:
        lg = masked_decoder(ids, mask, enc, P, c)[:, -1].double().numpy()
        col = []
        for b in range(B):
            if b not in live:
                col.append(R.EOS)
                continue
            x = lg[b].copy()
            if not gen[b]:
                x[list(R.BEGIN_SUPPRESS)] = -np.inf
            tok = R.pick(R.timestamp_rules(x, gen[b], R.TIMESTAMP_BEGIN, R.EOS, R.MAX_INITIAL_TIMESTAMP_INDEX))
            gen[b].append(tok)
            col.append(tok)
            if tok == R.EOS:
                live.remove(b)
        ids = torch.cat([ids, torch.tensor(col)[:, None]], 1)
        mask = torch.cat([mask, torch.ones(B, 1, dtype=torch.bool)], 1)
    return gen
