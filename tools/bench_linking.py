#!/usr/bin/env python3
"""Tubelet linking (detect_to_track/viterbi.py on the device): time of one problem and of a batch of 30 problems in one call,
at the four sizes of the reference's CPU timing (frames x detections per frame: 32 x 32, 64 x 64, 128 x 64, 128 x 128), beside
the numpy restatement's CPU time for one problem (tests/link_reference.py; the reference's pure-Python code is slower still).

Problems are seeded, as in the tests: random confidences, boxes, and about one track per detection near the detections.
Device times are host wall clock around link_batched (link scores + every extraction, offsets uploaded, nothing read back)
ending in a device synchronise, median of --reps after one warm-up.  One JSON line per size.

    python tools/bench_linking.py [--reps 5] [--out FILE]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "detect-to-track_amd", ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))
from detect_to_track import viterbi as V  # noqa: E402
import link_reference as L  # noqa: E402

SIZES = [(32, 32), (64, 64), (128, 64), (128, 128)]


def problem(rng, T, D):
    d = [int(x) for x in rng.integers(D // 2, 3 * D // 2 + 1, T)]      # about D per frame
    confs = [rng.random(n).astype(np.float32) for n in d]
    boxes = [np.concatenate([rng.uniform(0.2, 0.8, (n, 2)), rng.uniform(0.05, 0.4, (n, 2))], 1).astype(np.float32) for n in d]
    tracks = []
    for t in range(T - 1):
        tr = boxes[t][rng.integers(0, d[t], d[t])] + rng.normal(0, 0.03, (d[t], 4)).astype(np.float32)
        tr[:, 2:] = np.abs(tr[:, 2:])
        tracks.append(tr.astype(np.float32))
    return confs, boxes, tracks


def pack(problems, dev):
    c = torch.from_numpy(np.concatenate([x for p in problems for x in p[0]])).to(dev)
    b = torch.from_numpy(np.concatenate([x for p in problems for x in p[1]])).to(dev)
    t = torch.from_numpy(np.concatenate([x for p in problems for x in p[2]]).reshape(-1, 4)).to(dev)
    D = [len(x) for p in problems for x in p[0]]
    TC = [len(x) for p in problems for x in p[2]]
    FC = [len(p[0]) for p in problems]
    return c, b, t, D, TC, FC


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--iou", type=float, default=0.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_linking needs a GPU")
    dev = torch.device("cuda", 0)
    lines = []
    for T, D in SIZES:
        rng = np.random.default_rng(T * 1000 + D)
        probs = [problem(rng, T, D) for _ in range(30)]
        one, batch = pack(probs[:1], dev), pack(probs, dev)
        _, _, res = V.link_batched(*one, args.iou)
        n_tubelets = len(res.paths(0))
        t_one = timed(lambda: V.link_batched(*one, args.iou), args.reps)
        t_batch = timed(lambda: V.link_batched(*batch, args.iou), args.reps)
        c, b, t = probs[0]
        t0 = time.perf_counter()
        want = L.tracking(c, b, t, args.iou, 1)
        t_cpu = time.perf_counter() - t0
        assert len(want) == n_tubelets
        rec = dict(frames=T, dets_per_frame=D, tubelets_problem0=n_tubelets, device_s_per_problem=t_one,
                   device_s_batch30=t_batch, device_s_per_problem_in_batch=t_batch / 30, cpu_restatement_s_per_problem=t_cpu,
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
