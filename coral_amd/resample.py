"""Sampling-rate conversion on the GPU: audio at any rate into the model's 16 kHz path.

The reference's first step on every dataset is `dataset.cast_column("audio", Audio(sampling_rate=...))`
(R/src/coral/data.py, R/src/coral/validation.py); its demo resamples microphone input with libsamplerate.  Here the
host designs a polyphase table in float64 (`plan`) and `ca_resample` (csrc/resample.hip) applies it to a staged batch,
in front of `ca_pcm_prepare`.

The resampler is a band-limited Hann-windowed sinc interpolator at the rational ratio Nw / O (g = gcd(src, dst),
O = src / g, Nw = dst / g), the formula of `torchaudio.functional.resample` (`sinc_interp_hann`) without its all-zero
taps; with s = rolloff * min(1, Nw / O) and L = lowpass_filter_width,

    y[n] = sum over the integers m with |(m - n O / Nw) s| < L of
           x[m] * s * sinc((m - n O / Nw) s) * cos^2(pi (m - n O / Nw) s / (2 L)),

x[m] = 0 outside the recording, n_out = ceil(Nw * len / O), no renormalisation of the DC gain.  Parity with soxr
(`soxr_hq`, what `datasets` 3.x resamples with through librosa) and with libsamplerate is not pinned: neither is
installed beside this project.
"""

from __future__ import annotations

import math
import numbers
from dataclasses import dataclass, field

import numpy as np

from . import _lib

DEFAULT_WIDTH, DEFAULT_ROLLOFF = 32, 0.99  # (torchaudio's own default width is 6: selectable)


@dataclass(frozen=True)
class ResamplePlan:
    """The polyphase table of one (src, dst, width, rolloff): phase i = n mod Nw starts at input sample
    (n // Nw) * O + off[i] and has the taps taps[i, :K] (rows zero-padded to the largest support K)."""

    src: int
    dst: int
    lowpass_filter_width: int
    rolloff: float
    O: int
    Nw: int
    K: int
    off: np.ndarray   # int32 [Nw]
    taps: np.ndarray  # float32 [Nw, K]
    _device: dict = field(default_factory=dict, repr=False, compare=False)

    def out_length(self, n: int) -> int:
        """ceil(Nw * n / O): the samples `n` input samples become."""
        n = int(n)
        return 0 if n <= 0 else -((-self.Nw * n) // self.O)

    def in_length_for(self, n_out: int) -> int:
        """The longest input whose resampled length is at most `n_out`."""
        return (int(n_out) * self.O) // self.Nw

    def device_tables(self, device):
        """(taps, off) on `device`, uploaded once per device."""
        import torch

        dev = torch.device(device)
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        hit = self._device.get(key)
        if hit is None:
            hit = self._device[key] = (torch.from_numpy(self.taps).to(dev), torch.from_numpy(self.off).to(dev))
        return hit


_PLANS: dict = {}


def _rate(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or v != int(v):
        raise ValueError(f"{what} must be an integer number of Hz, got {v!r}")
    if int(v) <= 0:
        raise ValueError(f"{what} must be positive, got {v!r}")
    return int(v)


def plan(src, dst, lowpass_filter_width: int = DEFAULT_WIDTH, rolloff: float = DEFAULT_ROLLOFF) -> ResamplePlan:
    """The table that takes `src` Hz to `dst` Hz (cached; its device copies are cached per device on the plan)."""
    src, dst = _rate(src, "the source sampling rate"), _rate(dst, "the target sampling rate")
    if isinstance(lowpass_filter_width, bool) or lowpass_filter_width != int(lowpass_filter_width) or lowpass_filter_width < 1:
        raise ValueError(f"lowpass_filter_width must be an integer >= 1, got {lowpass_filter_width!r}")
    L, rolloff = int(lowpass_filter_width), float(rolloff)
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"rolloff must be in (0, 1], got {rolloff!r}")
    key = (src, dst, L, rolloff)
    hit = _PLANS.get(key)
    if hit is not None:
        return hit
    if src == dst:  # an exact copy: how the rows already at the target rate get into the fp32 buffer
        p = ResamplePlan(src, dst, L, rolloff, 1, 1, 1, np.zeros(1, np.int32), np.ones((1, 1), np.float32))
        _PLANS[key] = p
        return p
    g = math.gcd(src, dst)
    O, Nw = src // g, dst // g
    s = rolloff * min(1.0, Nw / O)
    half = L / s  # the support is |m - p| < half
    k_upper = 2 * int(math.ceil(half)) + 1
    if k_upper - 2 > _lib.RESAMPLE_MAX_TAPS:
        raise ValueError(f"resampling {src} -> {dst} Hz at lowpass_filter_width {L} needs about {k_upper} taps a phase, "
                         f"the limit is {_lib.RESAMPLE_MAX_TAPS} (CA_RESAMPLE_MAX_TAPS)")
    if Nw * (k_upper - 2) > _lib.RESAMPLE_MAX_TABLE:
        raise ValueError(f"resampling {src} -> {dst} Hz at lowpass_filter_width {L} needs a table of {Nw} phases x about "
                         f"{k_upper} taps, the limit is {_lib.RESAMPLE_MAX_TABLE} taps (CA_RESAMPLE_MAX_TABLE)")
    i = np.arange(Nw, dtype=np.int64)
    base = (i * O) // Nw
    d = np.arange(-int(math.ceil(half)) - 2, int(math.ceil(half)) + 4, dtype=np.int64)
    m = base[:, None] + d[None, :]
    t = (m * Nw - (i * O)[:, None]).astype(np.float64) / Nw * s  # (m - p_i) s, the numerator an exact integer
    inside = np.abs(t) < L
    first = inside.argmax(axis=1)
    count = inside.sum(axis=1)
    K = int(count.max())
    h = np.where(inside, s * np.sinc(t) * np.cos(np.pi * t / (2 * L)) ** 2, 0.0)
    taps = np.zeros((Nw, K), np.float64)
    for ph in range(Nw):
        taps[ph, :count[ph]] = h[ph, first[ph]:first[ph] + count[ph]]
    off = (m[i, first]).astype(np.int32)
    if K > _lib.RESAMPLE_MAX_TAPS:
        raise ValueError(f"resampling {src} -> {dst} Hz needs {K} taps a phase, the limit is {_lib.RESAMPLE_MAX_TAPS} "
                         "(CA_RESAMPLE_MAX_TAPS)")
    if Nw * K > _lib.RESAMPLE_MAX_TABLE:
        raise ValueError(f"resampling {src} -> {dst} Hz needs a table of {Nw} x {K} taps, the limit is "
                         f"{_lib.RESAMPLE_MAX_TABLE} (CA_RESAMPLE_MAX_TABLE)")
    window = 4 * (-((-_lib.RESAMPLE_CHUNK * O) // Nw) + K + 1)
    if window > _lib.RESAMPLE_LDS_BYTES:
        raise ValueError(f"resampling {src} -> {dst} Hz: the input window of one chunk of {_lib.RESAMPLE_CHUNK} outputs takes "
                         f"{window} bytes, the limit is {_lib.RESAMPLE_LDS_BYTES} (CA_RESAMPLE_LDS_BYTES)")
    p = ResamplePlan(src, dst, L, rolloff, O, Nw, K, off, taps.astype(np.float32))
    _PLANS[key] = p
    return p


def _as_pcm(a, i: int) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 1:
        raise ValueError(f"resample: array {i} has shape {a.shape}; multi-channel audio is not supported, pass one channel "
                         "(1-D int16 or float32 samples)")
    if a.dtype == np.int16 or a.dtype == np.float32:
        return a
    if a.dtype == np.float64 or a.dtype == np.float16:
        return a.astype(np.float32)
    raise ValueError(f"resample: array {i} has dtype {a.dtype}; expected int16 or float32 samples")


def rates_of(sampling_rate, n: int, default: int | None = None) -> list[int]:
    """One rate per recording from an int, a sequence of `n`, or None (= `default`)."""
    if sampling_rate is None:
        if default is None:
            raise ValueError("no sampling rate given")
        return [int(default)] * n
    if isinstance(sampling_rate, numbers.Real):
        return [_rate(sampling_rate, "sampling_rate")] * n
    rates = [_rate(default if r is None else r, "sampling_rate") for r in sampling_rate]
    if len(rates) != n:
        raise ValueError(f"{len(rates)} sampling rates for {n} recordings")
    return rates


def launch(src, len_in, y, len_out, rates, target, lowpass_filter_width=DEFAULT_WIDTH, rolloff=DEFAULT_ROLLOFF, route=0):
    """Enqueue ca_resample on the rows 0 .. len(rates)-1 of the staged batch `src` (int16 / fp32 [B, ld_in], device) with
    the lengths `len_in`, into `y` fp32 [B, ld_out] and `len_out`: one launch per distinct rate, the identity plan for
    the rows already at `target`."""
    import torch

    from . import ops

    by_rate: dict[int, list[int]] = {}
    for i, r in enumerate(rates):
        by_rate.setdefault(int(r), []).append(i)
    for r, idx in by_rate.items():
        p = plan(r, target, lowpass_filter_width, rolloff)
        taps, off = p.device_tables(src.device)
        rows = None if len(by_rate) == 1 else torch.tensor(idx, dtype=torch.int32).to(src.device, non_blocking=True)
        ops.resample(src, len_in, rows, len(idx), taps, off, p.O, p.Nw, p.K, y, len_out, route=route)


def resample(arrays, sampling_rate, target: int = 16_000, device="cuda", lowpass_filter_width: int = DEFAULT_WIDTH,
             rolloff: float = DEFAULT_ROLLOFF, to_host: bool = True):
    """Resample a ragged list of 1-D int16 / float32 recordings from `sampling_rate` (one int, or one per recording) to
    `target` Hz on the GPU.  -> a list of float32 arrays (or of device tensors with to_host=False).  The recordings are
    packed into one staging buffer and served by one launch per distinct rate."""
    import torch

    arrays = [_as_pcm(a, i) for i, a in enumerate(arrays)]
    rates = rates_of(sampling_rate, len(arrays))
    target = _rate(target, "the target sampling rate")
    plans = [plan(r, target, lowpass_filter_width, rolloff) for r in rates]
    if not arrays:
        return []
    if not torch.cuda.is_available():
        raise _lib.CoralAmdError("resample needs a GPU (there is no CPU path)")
    as_int16 = all(a.dtype == np.int16 for a in arrays)
    B, ld_in = len(arrays), max(1, max(len(a) for a in arrays))
    if ld_in >= 1 << 31:
        raise ValueError(f"resample: a recording of {ld_in} samples is above the 2^31 - 1 a row holds")
    n_out = [p.out_length(len(a)) for p, a in zip(plans, arrays)]
    ld_out = max(1, max(n_out))
    host = np.zeros((B, ld_in), np.int16 if as_int16 else np.float32)
    for i, a in enumerate(arrays):
        host[i, :len(a)] = a if as_int16 or a.dtype != np.int16 else a.astype(np.float32) * np.float32(1.0 / 32768.0)
    dev = torch.device(device)
    src = torch.from_numpy(host).to(dev)
    len_in = torch.tensor([len(a) for a in arrays], dtype=torch.int32).to(dev)
    y = torch.empty(B, ld_out, dtype=torch.float32, device=dev)
    len_out = torch.empty(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        launch(src, len_in, y, len_out, rates, target, lowpass_filter_width, rolloff)
    if not to_host:
        return [y[i, :n] for i, n in enumerate(n_out)]
    got = len_out.cpu().tolist()
    if got != n_out:
        raise _lib.CoralAmdError(f"ca_resample wrote the lengths {got}, the host expected {n_out}")
    y = y.cpu().numpy()
    return [y[i, :n].copy() for i, n in enumerate(n_out)]


def to_rate(audios, sampling_rate, target: int, device="cuda"):
    """What the callers that take `sampling_rate=` do first: the recordings unchanged when every rate is `target` (or
    none is given), else all of them through `resample` (the rows at `target` are exact copies, as float32)."""
    if sampling_rate is None:
        return audios
    rates = rates_of(sampling_rate, len(audios), default=target)
    if all(r == target for r in rates):
        return audios
    return resample(audios, rates, target=target, device=device)
