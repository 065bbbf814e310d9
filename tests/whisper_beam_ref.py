"""Plain-torch restatement of the beam search `WhisperEngine.generate(num_beams=k)` implements:
`GenerationMixin._beam_search` of the installed transformers ($TF/generation/utils.py:3208-3508) with Whisper's two
suppress processors, stated on small tensors so that one step can be compared with the device kernels.

What the restatement fixes beyond the source: `torch.topk` leaves the order of equal scores open; here ties go to
the lower flat index (beam * V + token; lower position in a merged list) - a stable descending sort.

  * per step: fp32 log_softmax of the logits, the suppress sets as -inf AFTER it (:3388-3389), + the running score
    (:3419), the top 2k of a clip's k * V candidates (:3113);
  * a candidate "hits" when its token is EOS or the sequence reaches max_length (the stopping criteria, :3438);
  * the best k by score + hit * -1e9 run on (:3145-3150);
  * hits among the first k ranks enter the clip's finished table with score / (generated_length ** length_penalty),
    generated_length = cur_len + 1 - prompt_len counting the EOS (:3182), unless the table is full and
    early_stopping is True (:3184) or the clip's heuristic has been satisfied (:3187); the table keeps its best k;
  * heuristic (:3047-3052, sticky): running best / ((cur_len - prompt_len) ** length_penalty) with the NEW cur_len
    must exceed the table's lowest score (-1e9 while the table has an empty place);
  * the loop ends when no clip's heuristic is unsatisfied, or early_stopping is True and every table is full, or every
    candidate hit (:3065-3075); the best finished hypothesis of each clip is returned, padded with pad_token_id.
"""
from __future__ import annotations

import numpy as np
import torch

NEG = -1.0e9


def rank_candidates(scores: np.ndarray, n: int) -> np.ndarray:
    """Indices of the best n entries of each row of `scores` [rows, m]: higher score first, then the lower index."""
    return np.argsort(-scores.astype(np.float32), axis=1, kind="stable")[:, :n]


def _topk(x: torch.Tensor, n: int):
    v, i = torch.sort(x, dim=1, descending=True, stable=True)
    return v[:, :n], i[:, :n]


def _gather(t: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    while idx.dim() < t.dim():
        idx = idx.unsqueeze(-1)
    return torch.gather(t, 1, idx.expand(*idx.shape[:2], *t.shape[2:]))


class BeamState:
    """The tensors _beam_search carries from step to step (B clips, k beams, sequences of max_length)."""

    def __init__(self, prefix: list[int], B: int, k: int, max_length: int, pad_id: int):
        P = len(prefix)
        self.B, self.k, self.P, self.max_length, self.cur = B, k, P, max_length, P
        self.running = torch.full((B, k, max_length), pad_id, dtype=torch.int64)
        self.running[:, :, :P] = torch.tensor(prefix)
        self.sequences = self.running.clone()
        self.running_scores = torch.zeros(B, k, dtype=torch.float32)
        self.running_scores[:, 1:] = NEG
        self.beam_scores = torch.full((B, k), NEG, dtype=torch.float32)
        self.lengths = torch.zeros(B, k, dtype=torch.int64)  # tokens of a finished hypothesis (EOS counted), 0 = none
        self.finished = torch.zeros(B, k, dtype=torch.bool)
        self.unsat = torch.ones(B, 1, dtype=torch.bool)
        self.all_hit = False


def select(log_probs: torch.Tensor, running_scores: torch.Tensor):
    """log_probs fp32 [B, k, V] (suppress applied) -> ranked (score, parent, token), each [B, 2k]."""
    B, k, V = log_probs.shape
    acc = (log_probs + running_scores[:, :, None]).reshape(B, k * V)
    s, i = _topk(acc, 2 * k)
    return s, i // V, i % V


def advance(st: BeamState, cand_score, cand_parent, cand_token, eos_id: int, length_penalty: float, early_stopping: bool):
    """One step of bookkeeping from the ranked candidates; returns (parent, token, score) of the new running beams."""
    B, k, P, cur = st.B, st.k, st.P, st.cur
    topk_seq = _gather(st.running, cand_parent).clone()
    topk_seq[:, :, cur] = cand_token
    hits = (cand_token == eos_id) | (cur + 1 >= st.max_length)
    run_lp = cand_score + hits.to(torch.float32) * NEG
    new_scores, nidx = _topk(run_lp, k)
    st.running = _gather(topk_seq, nidx)
    st.running_scores = new_scores
    parent, token = torch.gather(cand_parent, 1, nidx), torch.gather(cand_token, 1, nidx)
    # finished hypotheses
    top_mask = torch.arange(2 * k) < k
    did = hits & top_mask[None, :]
    fs = cand_score / ((cur + 1 - P) ** length_penalty)
    full = torch.all(st.finished, dim=-1, keepdim=True) & (early_stopping is True)
    fs = fs + full.to(torch.float32) * NEG
    fs = fs + (~st.unsat).to(torch.float32) * NEG
    fs = fs + (~did).to(torch.float32) * NEG
    merged_scores = torch.cat((st.beam_scores, fs), dim=1)
    _, midx = _topk(merged_scores, k)
    st.sequences = _gather(torch.cat((st.sequences, topk_seq), dim=1), midx)
    st.beam_scores = torch.gather(merged_scores, 1, midx)
    st.lengths = torch.gather(torch.cat((st.lengths, torch.full((B, 2 * k), cur + 1)), dim=1), 1, midx)
    st.finished = torch.gather(torch.cat((st.finished, did), dim=1), 1, midx)
    st.lengths = torch.where(st.finished, st.lengths, torch.zeros_like(st.lengths))
    st.cur = cur + 1
    best = st.running_scores[:, :1] / ((st.cur - P) ** length_penalty)
    worst = torch.where(st.finished, torch.min(st.beam_scores, dim=1, keepdim=True)[0], torch.tensor(NEG))
    st.unsat = st.unsat & torch.any(best > worst, dim=-1, keepdim=True)
    st.all_hit = bool(torch.all(hits))
    return parent, token, new_scores


def clip_done(st: BeamState, early_stopping: bool) -> torch.Tensor:
    """[B] bool: nothing can change in the clip's finished table any more."""
    return (~st.unsat[:, 0]) | (torch.all(st.finished, dim=-1) & (early_stopping is True)) | (st.cur >= st.max_length)


def search_over(st: BeamState, early_stopping: bool) -> bool:
    improvement_possible = bool(torch.any(st.unsat))
    exists_open_beam = not (bool(torch.all(st.finished)) and early_stopping is True)
    return not (improvement_possible and exists_open_beam and not st.all_hit)


def masked_log_probs(logits: torch.Tensor, cur: int, P: int, suppress, begin_suppress) -> torch.Tensor:
    lp = torch.log_softmax(logits.to(torch.float32), dim=-1)
    if suppress:
        lp[..., list(suppress)] = float("-inf")
    if begin_suppress and cur == P:
        lp[..., list(begin_suppress)] = float("-inf")
    return lp


def beam_search(logits_fn, prefix: list[int], B: int, num_beams: int, max_length: int, eos_id: int, pad_id: int,
                suppress=None, begin_suppress=None, length_penalty: float = 1.0, early_stopping: bool = False):
    """logits_fn(prefixes int64 [B * k, cur]) -> fp32 logits [B * k, V] of the last position.  Returns
    dict(sequences [B, n] (padded), scores [B], trace=[(parent, token, running score) per step, each [B, k]], state)."""
    k = num_beams
    st = BeamState(prefix, B, k, max_length, pad_id)
    trace = []
    while True:
        logits = logits_fn(st.running[:, :, :st.cur].reshape(B * k, st.cur))
        lp = masked_log_probs(logits, st.cur, st.P, suppress, begin_suppress).reshape(B, k, -1)
        trace.append(advance(st, *select(lp, st.running_scores), eos_id, length_penalty, early_stopping))
        if search_over(st, early_stopping):
            break
    n = int(st.lengths[:, 0].max())
    return dict(sequences=st.sequences[:, 0, :n], scores=st.beam_scores[:, 0], trace=trace, state=st)


# ---- the fixtures of tests/golden/whisper_beam.npz --------------------------------------------------------------------
MAX_LENGTH = 24
# the fixtures and cases of tools/gen_goldens.py (WHISPER_BEAM_FIXTURES / WHISPER_BEAM_CASES), restated
TINY = dict(d_model=64, encoder_layers=2, decoder_layers=2, encoder_attention_heads=4, decoder_attention_heads=4,
            encoder_ffn_dim=128, decoder_ffn_dim=128, num_mel_bins=80, vocab_size=200, max_target_positions=64,
            pad_token_id=150, decoder_start_token_id=151, eos_token_id=150)
MID = dict(d_model=512, encoder_layers=6, decoder_layers=6, encoder_attention_heads=8, decoder_attention_heads=8,
           encoder_ffn_dim=2048, decoder_ffn_dim=2048, num_mel_bins=80, vocab_size=2000, max_target_positions=64,
           pad_token_id=1950, decoder_start_token_id=1951, eos_token_id=1950)
FIXTURES = {
    "tiny": (TINY, 9, [151, 160, 161, 162], [170, 171], [20, 150]),
    "tiny_eos18": (dict(TINY, eos_token_id=18), 9, [151, 160, 161, 162], [170, 171], [20, 150]),
    "mid": (MID, 11, [1951, 1960, 1961, 1962], [1970, 1971], [20, 1950]),
    "mid_eos795": (dict(MID, eos_token_id=795), 11, [1951, 1960, 1961, 1962], [1970, 1971], [20, 1950]),
}
CASES = [(2, 1.0, False), (5, 1.0, False), (5, 1.0, True), (5, 0.6, False), (2, 0.6, True)]


def fixture(name):
    """-> (kw, config, params, features, prefix, suppress, begin_suppress) of a whisper_beam fixture."""
    from oracle import whisper_ref as w

    kw, seed, prefix, sup, sup_begin = FIXTURES[name]
    c = w.WhisperConfig(**kw)
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn(2, 80, 3000, generator=g) * 0.5
    return kw, c, w.synth_params(c), feats, prefix, sup, sup_begin
