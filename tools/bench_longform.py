#!/usr/bin/env python3
"""Audio-seconds per second of long-form wav2vec2 transcription (not bench.py: a side measurement).

One synthetic recording of `--minutes` minutes at the wav2vec2-small shape (XLS-R-300M, seeded random weights, V = 46)
through `coral_amd.longform.transcribe_long(chunk_length_s=10, batch_size=16)` with word timestamps: host wall-clock
around the whole call (host -> device copy of the recording, per-batch ca_pcm_prepare + forward + ca_ctc_stitch,
ca_ctc_collapse_offsets, the device-to-host copy, decoding on the host), synchronised, median of `--iters` calls after one
warm-up call.  `--whole` runs the same recording through the whole-clip path (`evaluate.transcribe(chunk_length_s=0)`)
instead - one forward over every frame - if the device holds its workspace.  One JSON line at the end.

    python tools/bench_longform.py [--minutes 10] [--iters 3] [--whole]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CHARS = "abcdefghijklmnopqrstuvwxyzæøå0123456789éü"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--chunk", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--whole", action="store_true")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_longform.py measures on the GPU; none is visible")
    from coral_amd.evaluate import transcribe
    from coral_amd.modeling import Wav2Vec2ForCTC
    from coral_amd.processor import CTCTokenizer, Wav2Vec2Processor, WaveformFeatureExtractor
    from coral_amd.wav2vec2 import CORAL_W2V2_SHAPES, Wav2Vec2Shape

    model = Wav2Vec2ForCTC(Wav2Vec2Shape(**CORAL_W2V2_SHAPES["wav2vec2-small"], vocab_size=46, pad_token_id=45), "cuda:0")
    model.init_weights(4242)
    model.eval()
    proc = Wav2Vec2Processor(WaveformFeatureExtractor(), CTCTokenizer({c: i for i, c in enumerate(sorted(set(CHARS + "|")))}))
    rng = np.random.RandomState(600)
    n = int(args.minutes * 60 * 16000)
    wave = np.clip(0.1 * rng.randn(n), -1, 1).astype(np.float32)
    kw = dict(chunk_length_s=0) if args.whole else dict(chunk_length_s=args.chunk, batch_size=args.batch,
                                                        return_timestamps="word")

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = transcribe(model, proc, [wave], **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    run()
    times = [run()[0] for _ in range(args.iters)]
    med = statistics.median(times)
    out = dict(path="whole_clip" if args.whole else "transcribe_long", minutes=args.minutes, audio_seconds=n / 16000,
               chunk_length_s=None if args.whole else args.chunk, batch_size=None if args.whole else args.batch,
               seconds_median=round(med, 4), seconds_min=round(min(times), 4), seconds_max=round(max(times), 4),
               audio_seconds_per_second=round(n / 16000 / med, 1),
               peak_memory_gb=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
