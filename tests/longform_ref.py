"""NumPy restatements for the long-form tests (no GPU, no transformers): the fixture waveform, the chunk stitch, the
CTC collapse with frame offsets (groupby run lengths, as `Wav2Vec2CTCTokenizer._compute_offsets`), and the fixture
loader shared by tests/test_longform_cpu.py and tests/test_longform_gpu.py."""
import json
from itertools import groupby
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
WAVE_SEED, WAVE_SECONDS, SAMPLING_RATE = 1729, 6.3, 16_000


def fixture_waveform(seed: int = WAVE_SEED, seconds: float = WAVE_SECONDS, sr: int = SAMPLING_RATE) -> np.ndarray:
    """Seeded noise under a piecewise-constant loudness envelope (50 ms steps), peak-normalised, fp32.  Only
    RandomState draws, multiplies and one division: the same bits wherever it is generated."""
    rng = np.random.RandomState(seed)
    n = int(round(seconds * sr))
    w = rng.randn(n)
    hop = sr // 20
    env = np.repeat(rng.uniform(0.05, 1.0, size=n // hop + 1), hop)[:n]
    w = (w * env).astype(np.float32)
    return w / np.abs(w).max()


_CACHE = {}


def load_fixture():
    """(json dict, npz) of tests/golden/w2v2_longform.*, loaded once."""
    if "fx" not in _CACHE:
        meta = json.loads((GOLDEN / "w2v2_longform.json").read_text())
        _CACHE["fx"] = (meta, np.load(GOLDEN / "w2v2_longform.npz"))
    return _CACHE["fx"]


def stitch_ref(logits: np.ndarray, seg, R: int, Tout: int, V: int, raw_fill: int, logits_fill: float):
    """logits [C, T, ldv], seg rows (row, off, left, keep) -> (raw [R, Tout], logits_out [R, Tout, ldv]) with the fills
    wherever nothing is written; np.argmax takes the first maximum."""
    C, T, ldv = logits.shape
    raw = np.full((R, Tout), raw_fill, np.int32)
    lo = np.full((R, Tout, ldv), logits_fill, np.float32)
    for c, (row, off, left, keep) in enumerate(seg):
        for j in range(keep):
            if left + j >= T:
                break
            raw[row, off + j] = int(np.argmax(logits[c, left + j, :V]))
            lo[row, off + j] = logits[c, left + j]
    return raw, lo


def collapse_ref(raw_row, in_len: int, blank: int):
    """One row -> (ids, start, end): every maximal run of equal ids inside [0, in_len) that is not blank, with its first
    frame and the first frame behind it."""
    ids, start, end, t = [], [], [], 0
    for k, grp in groupby(np.asarray(raw_row[:max(0, in_len)]).tolist()):
        n = len(list(grp))
        if k != blank:
            ids.append(k)
            start.append(t)
            end.append(t + n)
        t += n
    return ids, start, end


def collapse_ref_fast(raw_row: np.ndarray, in_len: int, blank: int):
    """collapse_ref vectorised (for rows of tens of thousands of frames)."""
    r = np.asarray(raw_row[:max(0, in_len)])
    if r.size == 0:
        return [], [], []
    rs = np.flatnonzero(np.concatenate(([True], r[1:] != r[:-1])))
    ends = np.concatenate((rs[1:], [r.size]))
    keep = r[rs] != blank
    return r[rs][keep].tolist(), rs[keep].tolist(), ends[keep].tolist()
