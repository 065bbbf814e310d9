"""The resampler of ca_resample without a GPU: the float64 restatement (tests/resample_ref.py) against
scipy.signal.upfirdn, coral_amd.resample.plan against the formula, the definition's sanity on tones, and the C ABI's
declaration and argument checks."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_ref as rref  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
RATES = (48_000, 44_100, 22_050, 11_025, 8_000)
# (K at L = 6, K at L = 32, phases) of src -> 16 kHz at rolloff 0.99
TABLES = {48_000: (37, 193, 1), 44_100: (34, 179, 160), 8_000: (13, 65, 2), 11_025: (13, 65, 640), 22_050: (17, 90, 320)}


@pytest.mark.parametrize("L", [6, 32])
@pytest.mark.parametrize("src", RATES)
def test_reference_against_upfirdn(src, L):
    signal = pytest.importorskip("scipy.signal")
    dst, rolloff = 16_000, 0.99
    O, Nw = rref.ratio(src, dst)
    s = rolloff * min(1.0, Nw / O)
    rng = np.random.default_rng(src + L)
    worst = 0.0
    for n in (300, 777, 2000):
        x = rng.standard_normal(n)
        y, _, _ = rref.resample(x, src, dst, L, rolloff, round_taps=False)
        Q = int(np.ceil(Nw * L / s))
        Q += (-Q) % O
        h = rref.kernel(np.arange(-Q, Q + 1, dtype=np.float64) / Nw, s, L)
        full = signal.upfirdn(h, x, up=Nw, down=O)
        got = full[Q // O:Q // O + len(y)]
        assert len(got) == len(y) == rref.out_length(n, src, dst)
        worst = max(worst, float(np.abs(got - y).max()))
    print(f"{src} -> {dst}, L = {L}: max |reference - upfirdn| = {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("L", [6, 32])
@pytest.mark.parametrize("src", RATES)
def test_plan_against_formula(src, L):
    from coral_amd import resample as rs

    p = rs.plan(src, 16_000, L, 0.99)
    O, Nw, K, off, taps = rref.phase_table(src, 16_000, L, 0.99)
    assert (p.O, p.Nw, p.K) == (O, Nw, K)
    assert (K, Nw) == (TABLES[src][0 if L == 6 else 1], TABLES[src][2])
    assert p.off.dtype == np.int32 and p.taps.dtype == np.float32 and p.taps.shape == (Nw, K) and p.off.shape == (Nw,)
    assert np.array_equal(p.off.astype(np.int64), off)
    assert np.all(np.abs(p.taps.astype(np.float64) - taps) <= 2.0 ** -24 * np.abs(taps) + 1e-12)
    if src == 44_100 and L == 6:
        assert (int(off.min()), int(off.max())) == (-16, 422)
    if src == 44_100:
        assert p.taps.nbytes == {6: 21_760, 32: 114_560}[L]
    if src == 11_025:
        assert p.taps.nbytes == {6: 33_280, 32: 166_400}[L]
    assert rs.plan(src, 16_000, L, 0.99) is p  # cached


def test_plan_identity_reduction_and_lengths():
    from coral_amd import resample as rs

    ident = rs.plan(16_000, 16_000)
    assert (ident.O, ident.Nw, ident.K) == (1, 1, 1)
    assert ident.off.tolist() == [0] and ident.taps.tolist() == [[1.0]] and ident.out_length(77) == 77
    half = rs.plan(32_000, 16_000)
    assert (half.O, half.Nw) == (2, 1)
    two = rs.plan(2, 1)
    assert two.K == half.K and np.array_equal(two.taps, half.taps) and np.array_equal(two.off, half.off)
    assert rs.plan(48_000, 16_000).lowpass_filter_width == 32 and rs.plan(48_000, 16_000).rolloff == 0.99  # the defaults
    assert [rs.plan(48_000, 16_000).out_length(n) for n in (0, 1, 2, 4)] == [0, 1, 1, 2]
    assert [rs.plan(44_100, 16_000).out_length(n) for n in (1, 3)] == [1, 2]
    assert rs.plan(8_000, 16_000).out_length(1) == 2
    big = rs.plan(48_000, 16_000).out_length(3_000_000_000)  # int64 arithmetic
    assert big == 1_000_000_000
    for src in RATES:
        p = rs.plan(src, 16_000)
        for n in (1, 2, 999, 16_001):
            assert p.out_length(n) == rref.out_length(n, src, 16_000)
            assert p.out_length(p.in_length_for(n)) <= n < p.out_length(p.in_length_for(n) + 1)


def test_plan_refusals_by_name():
    from coral_amd import resample as rs

    for bad in (0, -8000, 44_100.5, "16000", None, True):
        with pytest.raises(ValueError, match="sampling rate"):
            rs.plan(bad, 16_000)
        with pytest.raises(ValueError, match="sampling rate"):
            rs.plan(16_000, bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError, match="lowpass_filter_width"):
            rs.plan(48_000, 16_000, lowpass_filter_width=bad)
    for bad in (0.0, -0.5, 1.01):
        with pytest.raises(ValueError, match="rolloff"):
            rs.plan(48_000, 16_000, rolloff=bad)
    with pytest.raises(ValueError, match="CA_RESAMPLE_MAX_TAPS"):
        rs.plan(48_000, 16_000, lowpass_filter_width=1000)  # 2 * 1000 * 3 / 0.99 taps a phase
    with pytest.raises(ValueError, match="CA_RESAMPLE_MAX_TABLE"):
        rs.plan(15_999, 16_000, lowpass_filter_width=64)  # 16 000 phases of 130 taps
    with pytest.raises(ValueError, match="CA_RESAMPLE_LDS_BYTES"):
        rs.plan(1_600_000, 16_000, lowpass_filter_width=1)  # a chunk's window is 100 input samples per output
    with pytest.raises(ValueError, match="multi-channel"):
        rs.resample([np.zeros((2, 100), np.float32)], 48_000)
    with pytest.raises(ValueError, match="dtype"):
        rs.resample([np.zeros(100, np.int32)], 48_000)
    with pytest.raises(ValueError, match="2 sampling rates for 1"):
        rs.resample([np.zeros(100, np.float32)], [48_000, 16_000])
    assert rs.resample([], 48_000) == []


def test_definition_on_tones():
    """48 kHz -> 16 kHz at L = 32, fp32-rounded taps, 12 000 input samples, 400 output samples dropped at each end: a
    3 kHz unit sine comes out as the 3 kHz sine at 16 kHz (measured 6.4e-6), a 9 kHz sine (above the new Nyquist) vanishes
    (measured 3.7e-4).  The margins are wide on purpose: they catch a wrong scale s or window, not rounding."""
    t48 = np.arange(12_000, dtype=np.float64) / 48_000
    y3, _, _ = rref.resample(np.sin(2 * np.pi * 3000 * t48), 48_000, 16_000, 32, 0.99)
    assert len(y3) == 4000
    want = np.sin(2 * np.pi * 3000 * np.arange(4000, dtype=np.float64) / 16_000)
    e3 = float(np.abs(y3 - want)[400:-400].max())
    y9, _, _ = rref.resample(np.sin(2 * np.pi * 9000 * t48), 48_000, 16_000, 32, 0.99)
    e9 = float(np.abs(y9)[400:-400].max())
    print(f"3 kHz error {e3:.3e}, 9 kHz residue {e9:.3e}")
    assert e3 <= 1e-4 and e9 <= 1e-2


def test_c_abi_declared_and_checked_without_gpu():
    from coral_amd import _lib

    hdr = (ROOT / "include" / "coral_amd.h").read_text()
    assert "int ca_resample(" in hdr and "ca_resample" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ca_resample"][1]) == 16
    for name, value in (("CHUNK", _lib.RESAMPLE_CHUNK), ("MAX_TAPS", _lib.RESAMPLE_MAX_TAPS),
                        ("LDS_BYTES", _lib.RESAMPLE_LDS_BYTES)):
        assert int(re.search(rf"#define CA_RESAMPLE_{name} (\d+)", hdr).group(1)) == value
    assert "#define CA_RESAMPLE_MAX_TABLE (1 << 20)" in hdr and _lib.RESAMPLE_MAX_TABLE == 1 << 20
    lib = _lib.load()
    p = 4096  # any non-null value: every refusal below comes before the pointers are used

    def call(pcm=p, ld_in=100, len_in=p, rows=None, R=1, taps=p, off=p, O=3, Nw=1, K=37, y=p, ld_out=100, len_out=p, route=0):
        return lib.ca_resample(pcm, 0, ld_in, len_in, rows, R, taps, off, O, Nw, K, y, ld_out, len_out, route, None)

    cases = [
        (dict(pcm=None), b"null"), (dict(len_in=None), b"null"), (dict(taps=None), b"null"), (dict(off=None), b"null"),
        (dict(y=None), b"null"), (dict(len_out=None), b"null"),
        (dict(O=0), b"positive"), (dict(Nw=0), b"positive"), (dict(K=0), b"positive"), (dict(R=0), b"positive"),
        (dict(ld_out=0), b"positive"),
        (dict(K=4097), b"CA_RESAMPLE_MAX_TAPS"),
        (dict(Nw=1024, K=1025), b"Nw * K"),
        (dict(route=3), b"route"), (dict(route=-1), b"route"),
        (dict(route=1, O=441, Nw=640, K=65), b"route 1"),  # 11 025 Hz at L = 32: 166 400 bytes of taps
        (dict(O=200, Nw=1, K=100), b"window"),
    ]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        msg = lib.ca_last_error()
        assert b"ca_resample" in msg and word in msg, (kw, msg)
