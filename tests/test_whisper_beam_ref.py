"""Whisper beam search, CPU side: the restatement (tests/whisper_beam_ref.py) run over the fp32 oracle reproduces what
transformers' own beam search returned for the same weights and inputs (tests/golden/whisper_beam.npz, written by
`tools/gen_goldens.py whisper_beam`): ids exactly, sequence scores to 1e-5.  Plus the selection rule on hand-made tables
and the C ABI additions (no GPU needed)."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import whisper_beam_ref as bref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))

from whisper_beam_ref import CASES, FIXTURES, MAX_LENGTH, fixture  # noqa: E402


def oracle_logits_fn(P, c, enc, k):
    """prefixes [B * k, cur] -> the fp32 oracle's logits of the last position (row b * k + j reads clip b)."""
    from oracle import whisper_ref as w

    def fn(prefixes):
        with torch.no_grad():
            return w.decoder(prefixes, enc.repeat_interleave(k, dim=0), P, c)[:, -1].float()

    return fn


def test_the_generator_and_this_file_name_the_same_fixtures():
    import gen_goldens as gg

    assert gg.WHISPER_BEAM_CASES == CASES and gg.WHISPER_BEAM_MAX_LENGTH == MAX_LENGTH
    assert {k: tuple(v) for k, v in gg.WHISPER_BEAM_FIXTURES.items()} == FIXTURES


@pytest.mark.parametrize("name", list(FIXTURES))
def test_restatement_over_the_fp32_oracle_reproduces_transformers(golden_dir, name):
    from oracle import whisper_ref as w

    z = np.load(golden_dir / "whisper_beam.npz")
    kw, c, P, feats, prefix, sup, sup_begin = fixture(name)
    with torch.no_grad():
        enc = w.encoder(feats, P, c)
    for k, lp, es in CASES:
        key = f"{name}:k{k}:lp{lp}:es{int(es)}"
        r = bref.beam_search(oracle_logits_fn(P, c, enc, k), prefix, 2, k, MAX_LENGTH, c.eos_token_id, c.pad_token_id,
                             suppress=sup, begin_suppress=sup_begin, length_penalty=lp, early_stopping=es)
        assert r["sequences"].tolist() == z[key + ":ids"].tolist(), key
        err = np.abs(r["scores"].numpy() - z[key + ":scores"]).max()
        print(f"{key}: ids equal, sequence scores max-abs err {err:.2e}")
        assert err <= 1e-5, (key, err)


def test_a_fixture_clip_decodes_differently_under_beam_search(golden_dir):
    """Without this the GPU tests could not tell beam search from greedy decoding: clip 0 of whisper_mid (and of
    whisper_tiny) at num_beams = 5 leaves the greedy path (tests/golden/whisper_mid.npz / whisper_tiny.npz: same prefix,
    suppress sets and max_length)."""
    zb = np.load(golden_dir / "whisper_beam.npz")
    for name in ("mid", "tiny"):
        beam, greedy = zb[f"{name}:k5:lp1.0:es0:ids"], np.load(golden_dir / f"whisper_{name}.npz")["greedy_ids"]
        assert beam.shape == greedy.shape and (beam[0] != greedy[0]).any()
    # and the settings matter: early_stopping and the length penalty change what the EOS variants return
    assert zb["mid_eos795:k5:lp1.0:es0:ids"].shape != zb["mid_eos795:k5:lp1.0:es1:ids"].shape
    assert zb["tiny_eos18:k5:lp1.0:es0:ids"].shape != zb["tiny_eos18:k5:lp0.6:es0:ids"].shape


def test_selection_rule_on_hand_made_tables():
    """(score descending, flat index beam * V + token ascending) - a numpy stable sort over small tables with deliberate
    ties - is what `select` returns."""
    V, k = 6, 2
    lp = torch.tensor([[[-1.0, -2.0, -1.0, -3.0, -2.0, -9.0],
                        [-1.0, -1.0, -4.0, -2.0, -9.0, -9.0]]])
    run = torch.tensor([[0.0, 0.0]])
    s, parent, tok = bref.select(lp, run)
    flat = (lp + run[:, :, None]).reshape(1, k * V).numpy()
    want = bref.rank_candidates(flat, 2 * k)
    assert want.tolist() == [[0, 2, 6, 7]]  # the four -1.0: by flat index
    assert (parent * V + tok).tolist() == want.tolist() and s.tolist() == [[-1.0] * 4]
    # a running score moves a whole beam; -inf (suppressed) never ranks in front of a finite score
    lp2 = lp.clone()
    lp2[0, 0, 0] = float("-inf")
    s, parent, tok = bref.select(lp2, torch.tensor([[0.0, -0.5]]))
    assert (parent * V + tok).tolist() == [[2, 6, 7, 1]] and s.tolist() == [[-1.0, -1.5, -1.5, -2.0]]
    # the first step: [0, -1e9, ...] expands beam 0 only
    s, parent, tok = bref.select(lp, torch.tensor([[0.0, -1e9]]))
    assert parent.tolist() == [[0, 0, 0, 0]] and tok.tolist() == [[0, 2, 1, 4]]


def test_advance_finishes_only_eos_among_the_first_k_ranks():
    k, eos = 2, 5
    st = bref.BeamState([9], 1, k, 8, pad_id=0)
    # rank 0 is EOS (finishes), rank 3 is EOS outside the first k ranks (dropped from the running beams, not finished)
    cs = torch.tensor([[-1.0, -2.0, -3.0, -4.0]])
    parent, tok, sc = bref.advance(st, cs, torch.tensor([[0, 0, 0, 0]]), torch.tensor([[eos, 3, 4, eos]]), eos, 1.0, False)
    assert tok.tolist() == [[3, 4]] and sc.tolist() == [[-2.0, -3.0]]
    assert st.finished.tolist() == [[True, False]] and st.lengths.tolist() == [[2, 0]]
    assert st.sequences[0, 0, :2].tolist() == [9, eos] and float(st.beam_scores[0, 0]) == -1.0
    assert bool(st.unsat[0, 0])  # an empty place in the table: the search goes on


def test_c_abi_additions_are_declared_and_mirrored(tmp_path):
    """ca_beam_* in header, SIGNATURES and ops; CaBeamDesc and CaAttnDesc.key_slot laid out as g++ lays the header out."""
    from coral_amd import _lib, ops

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    for sym in ("ca_beam_select_workspace_bytes", "ca_beam_select", "ca_beam_advance"):
        assert re.search(rf"\b{sym}\s*\(", hdr) and sym in _lib.SIGNATURES
    for fn in ("beam_select_workspace_bytes", "beam_select", "beam_advance"):
        assert callable(getattr(ops, fn))
    src = tmp_path / "layout.cc"
    fields = [n for n, _ in _lib.CaBeamDesc._fields_]
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "coral_amd.h"\nint main() {\n'
                   + "".join(f'  std::printf("%zu\\n", offsetof(CaBeamDesc, {n}));\n' for n in fields)
                   + '  std::printf("%zu %zu %zu %d %d\\n", sizeof(CaBeamDesc), offsetof(CaAttnDesc, key_slot), '
                     'offsetof(CaAttnDesc, klen), CA_BEAM_MAX_BEAMS, CA_BEAM_MAX_ROWS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["g++", "-std=c++17", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    offs, (size, ks, kl, mb, mr) = [int(v) for v in out[:len(fields)]], [int(v) for v in out[len(fields):]]
    assert offs == [getattr(_lib.CaBeamDesc, n).offset for n in fields] and size == C.sizeof(_lib.CaBeamDesc)
    assert ks == _lib.CaAttnDesc.key_slot.offset == kl + 8
    assert (mb, mr) == (_lib.BEAM_MAX_BEAMS, _lib.BEAM_MAX_ROWS) == (16, 128)


def test_generate_refuses_what_it_does_not_implement():
    """Argument checks of the public generate (no GPU: they run before any device work)."""
    from coral_amd.whisper import check_beam_arguments

    check_beam_arguments(8, 5, 1.0, False, {})
    check_beam_arguments(8, 16, 0.6, True, {})
    with pytest.raises(ValueError, match="128"):
        check_beam_arguments(26, 5, 1.0, False, {})
    with pytest.raises(ValueError, match="16"):
        check_beam_arguments(1, 17, 1.0, False, {})
    for kw in (dict(num_return_sequences=2), dict(do_sample=True), dict(temperature=0.7), dict(top_k=5),
               dict(repetition_penalty=1.2), dict(num_beam_groups=2), dict(return_timestamps=True)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            check_beam_arguments(2, 5, 1.0, False, kw)
    with pytest.raises(ValueError, match="never"):
        check_beam_arguments(2, 5, 1.0, "never", {})
    with pytest.raises(ValueError, match="num_beams"):
        check_beam_arguments(2, 0, 1.0, False, {})
