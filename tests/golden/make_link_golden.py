#!/usr/bin/env python3
"""Generate the tubelet-linking fixtures tests/golden/link_*.npz from THE REFERENCE'S OWN viterbi.py.

    python tests/golden/make_link_golden.py <reference checkout> [out_dir]

The reference's linking code (detect_to_track/viterbi.py) is plain numpy and runs on the CPU; it is loaded from the
given checkout by file path and run unmodified.  It imports two helpers from `ml_utils`, which the reference does not
vendor; this script supplies them as a stub package:

  ml_utils.boundingboxes.compute_ious(a, b)   (|a|, |b|) float32 IoU of (centre_i, centre_j, h, w) boxes, the
                                              expression of oracle/regions.py:iou_one_to_many (the project's convention)
  ml_utils.sequence.sliding_window(it, n)     consecutive n-tuples

Each fixture holds seeded inputs and the reference's outputs (data only):

  kind            "tracking" (viterbi_tracking), "multi_link" (viterbi_multi_link) or "viterbi" (viterbi)
  D               (T,) int64 detections per frame
  confs, boxes    tracking: concatenated per-frame float32 confidences / boxes
  tracks, n_tracks tracking: concatenated per-pair float32 track boxes and their counts; iou_thresh, min_len
  mats            float64 bit patterns (uint64) of the T-1 transition matrices, concatenated row-major: the
                  reference's compute_score_seq output for "tracking", the input otherwise
  init, has_init  the init scores passed in (multi_link / viterbi; has_init = 0 for None)
  p_start, p_end, p_len, p_score (uint64 bit patterns), p_nodes (concatenated frame-local node indices)
                  every path the reference returns, in its order
  n_tubelets      tracking: how many of them viterbi_tracking keeps (length >= min_len)
  ref_sources_sha256   the source stamp every fixture here carries (make_golden.py), re-verified against the given checkout
  viterbi_sha256       sha256 of the checkout's detect_to_track/viterbi.py
"""
import hashlib
import importlib.util
import signal
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
OUT = ROOT / "tests" / "golden"

_STUB_BOXES = '''
import numpy as np

def compute_ious(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1, 4), np.asarray(b, np.float32).reshape(-1, 4)
    f = np.float32
    two = f(2)
    out = np.zeros((len(a), len(b)), np.float32)
    for i, box in enumerate(a):
        ai0, ai1, aj0, aj1 = box[0] - box[2] / two, box[0] + box[2] / two, box[1] - box[3] / two, box[1] + box[3] / two
        bi0, bi1 = b[:, 0] - b[:, 2] / two, b[:, 0] + b[:, 2] / two
        bj0, bj1 = b[:, 1] - b[:, 3] / two, b[:, 1] + b[:, 3] / two
        ih = np.minimum(ai1, bi1) - np.maximum(ai0, bi0)
        iw = np.minimum(aj1, bj1) - np.maximum(aj0, bj0)
        inter = np.where(ih > 0, ih, f(0)) * np.where(iw > 0, iw, f(0))
        uni = box[2] * box[3] + b[:, 2] * b[:, 3] - inter
        with np.errstate(divide="ignore", invalid="ignore"):
            out[i] = np.where(uni > 0, inter / uni, f(0))
    return out
'''
_STUB_SEQ = '''
def sliding_window(iterable, n):
    items = list(iterable)
    return [tuple(items[i:i + n]) for i in range(len(items) - n + 1)]
'''


def load_reference_viterbi(reference: Path):
    stub = Path(tempfile.mkdtemp(prefix="ml_utils_stub_"))
    (stub / "ml_utils").mkdir()
    (stub / "ml_utils" / "__init__.py").write_text("")
    (stub / "ml_utils" / "boundingboxes.py").write_text(_STUB_BOXES)
    (stub / "ml_utils" / "sequence.py").write_text(_STUB_SEQ)
    sys.path.insert(0, str(stub))
    spec = importlib.util.spec_from_file_location("reference_viterbi", reference / "detect_to_track" / "viterbi.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Hang(Exception):
    pass


def _bounded(fn, *args, seconds=10):
    """The reference loops forever where an extraction picks a removed node (include/d2t_ops.h, linking section):
    such draws are not fixtures.  Runs fn under an alarm and raises _Hang when it fires."""
    def fire(*_):
        raise _Hang()
    old = signal.signal(signal.SIGALRM, fire)
    signal.alarm(seconds)
    try:
        return fn(*args)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def source_stamps(reference: Path):
    """The kernel fixtures' stamp, checked file by file against this checkout, and the hash of its viterbi.py."""
    stamp = str(np.load(sorted(OUT.glob("corr_*.npz"))[0])["ref_sources_sha256"])
    for line in stamp.strip().splitlines():
        digest, name = line.split(None, 1)
        name = name.strip()
        path = ROOT / name if name.startswith("oracle/") else reference / "detect_to_track" / "models" / name
        assert hashlib.sha256(path.read_bytes()).hexdigest() == digest, f"{name} differs from the fixtures' stamp"
    return dict(ref_sources_sha256=np.asarray(stamp),
                viterbi_sha256=np.asarray(hashlib.sha256((reference / "detect_to_track" / "viterbi.py").read_bytes()).hexdigest()))


STAMPS = {}


def _bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _paths(paths):
    return dict(p_start=np.array([p[0][0] for p in paths], np.int64), p_end=np.array([p[0][1] for p in paths], np.int64),
                p_len=np.array([len(p[2]) for p in paths], np.int64), p_score=_bits([p[1] for p in paths]),
                p_nodes=np.array([n for p in paths for n in p[2]], np.int64))


def random_track_problem(rng, T, dmax, tie_levels=0, empty=()):
    D = [int(rng.integers(0, dmax + 1)) for _ in range(T)]
    for t in empty:
        D[t] = 0
    confs, boxes, tracks = [], [], []
    for t in range(T):
        c = rng.random(D[t]).astype(np.float32)
        if tie_levels:
            c = ((np.floor(c * tie_levels) + 1) / tie_levels).astype(np.float32)   # no zero confidence
        confs.append(c)
        boxes.append(np.concatenate([rng.uniform(0.2, 0.8, (D[t], 2)), rng.uniform(0.1, 0.5, (D[t], 2))], 1).astype(np.float32))
    for t in range(T - 1):
        # tracks near the detections of frame t (the tracker's regressed boxes), plus some strays
        n = int(rng.integers(0, D[t] + 3))
        base = boxes[t][rng.integers(0, D[t], n)] if D[t] else np.zeros((n, 4), np.float32)
        tr = base + rng.normal(0, 0.05, (n, 4)).astype(np.float32)
        tr[:, 2:] = np.abs(tr[:, 2:])
        tracks.append(tr.astype(np.float32).reshape(-1, 4))
    return confs, boxes, tracks


def save_tracking(ref, name, confs, boxes, tracks, iou, min_len):
    mats = ref.compute_score_seq(confs, boxes, tracks, iou)
    paths = _bounded(ref.viterbi_multi_link, mats, confs[0].tolist())
    tubes = _bounded(ref.viterbi_tracking, confs, boxes, tracks, iou, min_len)
    np.savez_compressed(
        OUT / f"link_{name}.npz", kind=np.asarray("tracking"), D=np.array([len(c) for c in confs], np.int64),
        confs=np.concatenate(confs).astype(np.float32), boxes=np.concatenate(boxes).reshape(-1, 4).astype(np.float32),
        tracks=(np.concatenate(tracks) if tracks else np.zeros((0, 4))).reshape(-1, 4).astype(np.float32),
        n_tracks=np.array([len(t) for t in tracks], np.int64), iou_thresh=np.float64(iou), min_len=np.int64(min_len),
        mats=_bits(np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0)), n_tubelets=np.int64(len(tubes)),
        **_paths(paths), **STAMPS)


def save_matrices(ref, name, kind, mats, init):
    D = ([len(init)] if init is not None else [mats[0].shape[0]]) + [m.shape[1] for m in mats]
    if kind == "viterbi":
        path, score = ref.viterbi([m.copy() for m in mats], None if init is None else list(init))
        paths = [((len(mats) - len(path) + 1, len(mats)), score, path)]
    else:
        keep = [m.copy() for m in mats]
        paths = _bounded(ref.viterbi_multi_link, mats, None if init is None else list(init))
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(keep, mats)), "the reference modified its input"
    np.savez_compressed(
        OUT / f"link_{name}.npz", kind=np.asarray(kind), D=np.array(D, np.int64),
        mats=_bits(np.concatenate([m.ravel() for m in mats]) if mats else np.zeros(0)),
        init=np.asarray(init if init is not None else [], np.float64), has_init=np.int64(init is not None), **_paths(paths), **STAMPS)


def main():
    global OUT
    ref = load_reference_viterbi(Path(sys.argv[1]))
    STAMPS.update(source_stamps(Path(sys.argv[1])))
    if len(sys.argv) > 2:
        OUT = Path(sys.argv[2])
        OUT.mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(20261015)
    for i, (T, dmax, iou) in enumerate([(2, 6, 0.5), (5, 8, 0.3), (8, 12, 0.5), (12, 10, 0.7), (16, 16, 0.5), (6, 24, 0.3)]):
        c, b, t = random_track_problem(rng, T, dmax)
        save_tracking(ref, f"rand{i}_T{T}_D{dmax}", c, b, t, iou, min_len=2)
    c, b, t = random_track_problem(rng, 1, 5)
    c[0] = c[0][:5] if len(c[0]) >= 5 else rng.random(5).astype(np.float32)
    b[0] = np.concatenate([rng.uniform(0.2, 0.8, (len(c[0]), 2)), rng.uniform(0.1, 0.5, (len(c[0]), 2))], 1).astype(np.float32)
    save_tracking(ref, "single_frame", c, b, t, 0.5, min_len=1)
    c, b, t = random_track_problem(rng, 9, 7, empty=(0, 3, 4, 8))
    save_tracking(ref, "empty_frames", c, b, t, 0.5, min_len=1)
    c, b, t = random_track_problem(rng, 10, 9, tie_levels=3)
    save_tracking(ref, "conf_ties", c, b, t, 0.3, min_len=3)
    # restarts after frame 0: negative links make a fresh start (score 0.0) beat every continuation
    def restarts(r):
        return [r.normal(0.2, 0.5, (d0, d1)) for d0, d1 in zip([4, 5, 3, 6, 4], [5, 3, 6, 4, 5])], r.normal(0, 0.5, 4)

    # caller -inf masks (and ties in the matrices): passed straight to viterbi_multi_link
    def masked(r):
        mats = []
        for d0, d1 in zip([6, 7, 5, 8, 6, 7], [7, 5, 8, 6, 7, 4]):
            m = (np.round(r.random((d0, d1)) * 4) + 1) / 4
            m[r.random((d0, d1)) < 0.4] = -np.inf
            mats.append(m)
        return mats, (np.round(r.random(6) * 4) + 1) / 4

    for name, draw, with_init in (("restarts", restarts, True), ("neginf_masks", masked, True), ("neginf_masks_noinit", masked, False)):
        for seed in range(100):                                      # the first draw the reference finishes
            mats, init = draw(np.random.default_rng([20261015, seed]))
            try:
                save_matrices(ref, name, "multi_link", mats, init if with_init else None)
                break
            except _Hang:
                continue
    # viterbi() alone: with init scores, without them, and with no transitions at all
    mats = [rng.random((d0, d1)) for d0, d1 in zip([5, 6, 4, 7], [6, 4, 7, 3])]
    save_matrices(ref, "viterbi_init", "viterbi", mats, rng.random(5))
    save_matrices(ref, "viterbi_noinit", "viterbi", mats, None)
    save_matrices(ref, "viterbi_one_frame", "viterbi", [], rng.random(6))


if __name__ == "__main__":
    main()
