#!/usr/bin/env python3
"""Time of the resampling kernel (ca_resample) and of the wav2vec2 input pipeline with and without it (not bench.py: a
side measurement).  HIP-event medians over `--iters` launches after 5 warm-ups.

  (a) ca_resample alone on `--clips` clips of `--seconds` s at 48 000 and 44 100 Hz -> 16 000 Hz: int16 and fp32 input,
      lowpass_filter_width 6 and 32, the table in LDS (route 1, where it fits) and in global memory (route 2), and what
      route 0 picks;
  (b) one `get()` of DeviceInputPipeline (wav2vec2, int16) on the same clips at 48 000 Hz with max_source_rate, and on
      clips of the same duration already at 16 000 Hz.
Every timed table is first checked on one row against a float64 evaluation of the definition.  One JSON line at the end.

    python tools/bench_resample.py [--iters 20] [--clips 8] [--seconds 10]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from coral_amd import _lib, ops  # noqa: E402
from coral_amd import resample as rs  # noqa: E402
from coral_amd.input_pipeline import DeviceInputPipeline  # noqa: E402

DEV = "cuda:0"


def event_median_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    return round(statistics.median(times), 1), round(min(times), 1), round(max(times), 1)


def spot_check(p, x, y, n_check=64):
    """Outputs spread over one row against the float64 sum of the table's own taps: (K + 2) 2^-23 sum |h x|."""
    x = x.astype(np.float64) / (32768.0 if x.dtype == np.int16 else 1.0)
    taps = p.taps.astype(np.float64)
    for n in np.linspace(0, len(y) - 1, n_check).astype(np.int64):
        m0 = (n // p.Nw) * p.O + int(p.off[n % p.Nw])
        idx = m0 + np.arange(p.K)
        ok = (idx >= 0) & (idx < len(x))
        prod = taps[n % p.Nw][ok] * x[idx[ok]]
        assert abs(float(y[n]) - prod.sum()) <= (p.K + 2) * 2.0 ** -23 * np.abs(prod).sum(), (int(n), float(y[n]), prod.sum())


def fits_lds(p):
    window = 4 * (-((-_lib.RESAMPLE_CHUNK * p.O) // p.Nw) + p.K + 1)
    return window + 4 * p.Nw * (p.K | 1) <= _lib.RESAMPLE_LDS_BYTES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    iters = max(20, args.iters)
    rng = np.random.RandomState(0)
    out = dict(device=torch.cuda.get_device_name(0), clips=args.clips, seconds=args.seconds, iters=iters, kernel_us={})
    for src in (48_000, 44_100):
        n = int(args.seconds * src)
        wave = np.clip(0.2 * rng.randn(args.clips, n), -1, 1)
        for dtype in (np.int16, np.float32):
            host = (wave * 32767).astype(np.int16) if dtype == np.int16 else wave.astype(np.float32)
            x = torch.from_numpy(host).to(DEV)
            len_in = torch.full((args.clips,), n, dtype=torch.int32, device=DEV)
            for L in (6, 32):
                p = rs.plan(src, 16_000, L)
                taps, off = p.device_tables(DEV)
                y = torch.empty(args.clips, p.out_length(n), dtype=torch.float32, device=DEV)
                len_out = torch.empty(args.clips, dtype=torch.int32, device=DEV)
                for route in (1, 2, 0):
                    if route == 1 and not fits_lds(p):
                        continue

                    def launch(route=route):
                        ops.resample(x, len_in, None, args.clips, taps, off, p.O, p.Nw, p.K, y, len_out, route=route)

                    launch()
                    torch.cuda.synchronize()
                    assert len_out.tolist() == [p.out_length(n)] * args.clips
                    spot_check(p, host[args.clips - 1], y[args.clips - 1].cpu().numpy())
                    key = f"{src}_{np.dtype(dtype).name}_L{L}_route{route}"
                    out["kernel_us"][key] = event_median_us(launch, iters)
                    print(key, out["kernel_us"][key], flush=True)
    # (b) one get() of the wav2vec2 pipeline
    n16, n48 = int(args.seconds * 16_000), int(args.seconds * 48_000)
    a16 = [(np.clip(0.2 * rng.randn(n16), -1, 1) * 32767).astype(np.int16) for _ in range(args.clips)]
    a48 = [(np.clip(0.2 * rng.randn(n48), -1, 1) * 32767).astype(np.int16) for _ in range(args.clips)]
    pipe = DeviceInputPipeline(DEV, args.clips, n16, dtype=np.int16, max_source_rate=48_000)
    plain = DeviceInputPipeline(DEV, args.clips, n16, dtype=np.int16)

    def timed_get(pp, audios, rate):
        # the same staged batch again and again: only get() (the device side) is inside the events
        times = []
        for i in range(5 + iters):
            pp.submit(audios, sampling_rate=rate)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pp.get()
            b.record()
            b.synchronize()
            if i >= 5:
                times.append(1e3 * a.elapsed_time(b))
        return round(statistics.median(times), 1), round(min(times), 1), round(max(times), 1)

    out["pipeline_get_us"] = dict(at_16000_plain=timed_get(plain, a16, None), at_16000_with_max_source_rate=timed_get(pipe, a16, 16_000),
                                  at_48000_resampled=timed_get(pipe, a48, 48_000))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
