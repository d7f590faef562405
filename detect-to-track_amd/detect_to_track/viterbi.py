"""Tubelet linking on the device: the reference's detect_to_track/viterbi.py with the same names, signatures and return
types (numpy in, lists / arrays out), run by the HIP kernels of libd2t_ops.so (csrc/d2t_link.hip).

    compute_link_scores(confs_a, confs_b, bboxes_a, bboxes_b, tracks, iou_thresh) -> (|A|, |B|) float64
    compute_score_seq(conf_seq, bbox_seq, track_seq, iou_thresh) -> [matrix, ...]
    viterbi(score_seq, init_scores=None) -> (path, score)
    viterbi_multi_link(score_seq, init_scores=None) -> [((start, end), score, path), ...]
    viterbi_tracking(conf_seq, bbox_seq, track_seq, iou_thresh, min_len) -> [((start, end), boxes), ...]

Results equal the reference's bit for bit (include/d2t_ops.h, linking section).  Where the reference raises, these raise
the same type: ValueError for mismatched sequence lengths or for no transitions without init scores, IndexError for a
single frame without detections.  Where the reference would loop forever (an extraction whose best final node was
already removed, e.g. all-zero scores), these raise RuntimeError.  Confidences and boxes must be float32 and score
matrices float64 (TypeError otherwise); matrices must chain, (D_t, D_t+1) then (D_t+1, D_t+2) (ValueError otherwise).
There is no CPU implementation: the work runs on the current CUDA device.

For many problems (classes x videos) at once, ``link_batched`` takes device tensors and runs every problem in one call
of each of the two library entry points.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .models import _ext, _native


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("detect_to_track.viterbi runs on the GPU: no CUDA device is available")
    return torch.device("cuda", torch.cuda.current_device())


def _f32(x, name):
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"{name} must be float32, got {x.dtype}")
    return x


class LinkResult:
    """Output of ``link_batched``: device tensors start, length, score, nodes (N,), count, status (P,) and the node offset of
    every problem (host).  ``paths(p)`` reads problem p back as the reference's list of ((start, end), score, path)."""

    def __init__(self, outs, node_start, max_paths):
        self.start, self.length, self.score, self.nodes, self.count, self.status = outs
        self.node_start = node_start
        self.max_paths = max_paths
        self._host = None

    def _fetch(self):
        if self._host is None:
            self._host = [t.cpu().numpy() for t in (self.start, self.length, self.score, self.nodes, self.count, self.status)]
        return self._host

    def check(self, p):
        st = int(self._fetch()[5][p])
        if st == _native.LINK_NONTERMINATING:
            raise RuntimeError(f"problem {p}: an extraction picks an already removed node; the reference's "
                               "viterbi_multi_link would repeat it forever")
        if st == _native.LINK_EMPTY:
            raise ValueError("max() arg is an empty sequence")
        if st != _native.LINK_OK:
            raise RuntimeError(f"problem {p}: linking failed with status {st}")

    def paths(self, p) -> List[Tuple[Tuple[int, int], float, List[int]]]:
        self.check(p)
        start, length, score, nodes, count, _ = self._fetch()
        n0 = int(self.node_start[p])
        out, pos = [], n0
        for k in range(int(count[p])):
            s, n = int(start[n0 + k]), int(length[n0 + k])
            out.append(((s, s + n - 1), float(score[n0 + k]), [int(v) for v in nodes[pos:pos + n]]))
            pos += n
        return out


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off


def _layout(frame_counts, det_counts, dev):
    """(det_off, frame_off, mat_off) device tensors, M, max_dets, max_frames, node offsets per problem (host)."""
    frame_counts, det_counts = np.asarray(frame_counts, np.int64), np.asarray(det_counts, np.int64)
    if (frame_counts < 1).any():
        raise ValueError("every problem needs at least one frame")
    if det_counts.size and det_counts.max() > _native.LINK_MAX_DETS:
        raise ValueError(f"at most {_native.LINK_MAX_DETS} detections per frame, got {int(det_counts.max())}")
    if frame_counts.size and frame_counts.max() > _native.LINK_MAX_FRAMES:
        raise ValueError(f"at most {_native.LINK_MAX_FRAMES} frames per problem, got {int(frame_counts.max())}")
    frame_off, det_off = _offsets(frame_counts), _offsets(det_counts)
    last = np.zeros(len(det_counts), bool)
    last[frame_off[1:] - 1] = True                                    # the last frame of a problem starts no pair
    sizes = (det_counts[:-1] * det_counts[1:])[~last[:-1]] if len(det_counts) > 1 else np.zeros(0, np.int64)
    mat_off = _offsets(sizes)
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
    return (to(det_off, np.int32), to(frame_off, np.int32), to(mat_off[:-1], np.int64), int(mat_off[-1]),
            int(det_counts.max()) if det_counts.size else 0, int(frame_counts.max()) if frame_counts.size else 0,
            det_off[frame_off[:-1]])


def link_batched(confs: torch.Tensor, boxes: torch.Tensor, tracks: torch.Tensor, det_counts: Sequence[int],
                 track_counts: Sequence[int], frame_counts: Sequence[int], iou_thresh: float, max_paths: int = 0,
                 init: Optional[torch.Tensor] = None):
    """viterbi_tracking's linking for P problems in one call of each library entry point.

    confs (N,), boxes (N,4), tracks (NT,4): float32 tensors on the device, the problems' frames one after another;
    det_counts (F,) detections per frame, track_counts (F-P,) tracks per adjacent frame pair, frame_counts (P,) frames per
    problem: host integers (they fix every output size).  init (N,) float64 on the device, read at frame-0 nodes, defaults
    to the frame-0 confidences as float64, as viterbi_tracking's init.  Returns (scores (M,) float64 device tensor of every
    pair's link matrix, status (1,) int32 of the link scores, LinkResult)."""
    for t, name in ((confs, "confs"), (boxes, "boxes"), (tracks, "tracks")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor")
    track_counts = np.asarray(track_counts, np.int64)
    if len(track_counts) != len(det_counts) - len(frame_counts):
        raise ValueError(f"need one track count per frame pair ({len(det_counts) - len(frame_counts)}), got {len(track_counts)}")
    if track_counts.size and track_counts.max() > _native.LINK_MAX_TRACKS:
        raise ValueError(f"at most {_native.LINK_MAX_TRACKS} tracks per frame pair, got {int(track_counts.max())}")
    dev = confs.device
    det_off, frame_off, mat_off, M, max_dets, max_frames, node_start = _layout(frame_counts, det_counts, dev)
    track_off = torch.from_numpy(_offsets(track_counts).astype(np.int32)).to(dev)
    scores, status = _ext.link_scores(confs, boxes, det_off, frame_off, tracks, track_off, mat_off, iou_thresh, M, max_dets,
                                      int(track_counts.max()) if track_counts.size else 0)
    if init is None:
        init = confs.double()
    outs = _ext.link_paths(scores, mat_off, init, det_off, frame_off, max_dets, max_frames, max_paths)
    return scores, status, LinkResult(outs, node_start, max_paths)


def link_matrices_batched(problems: Sequence[Tuple[Sequence[np.ndarray], Optional[Sequence[float]]]], max_paths: int = 0):
    """viterbi_multi_link (max_paths = 0) or viterbi (max_paths = 1) of many (score_seq, init_scores) problems in one launch.
    Matrices float64, chained; init None = zeros.  Returns a LinkResult."""
    det_counts, frame_counts, mats, inits = [], [], [], []
    for score_seq, init in problems:
        score_seq = list(score_seq)
        for m in score_seq:
            if not isinstance(m, np.ndarray) or m.dtype != np.float64 or m.ndim != 2:
                raise TypeError("score matrices must be 2-d float64 numpy arrays")
        d0 = len(init) if init else (score_seq[0].shape[0] if score_seq else None)
        if d0 is None:
            raise IndexError("list index out of range")              # the reference: score_seq[0] of an empty sequence
        D = [d0] + [m.shape[1] for m in score_seq]
        for t, m in enumerate(score_seq):
            if m.shape[0] != D[t]:
                raise ValueError(f"score matrix {t} has {m.shape[0]} rows, frame {t} has {D[t]} nodes")
        det_counts += D
        frame_counts.append(len(D))
        mats += [m.ravel() for m in score_seq]
        inits.append(np.asarray(init, np.float64) if init else np.zeros(d0))
        inits.append(np.zeros(sum(D[1:])))
    dev = _device()
    det_off, frame_off, mat_off, M, max_dets, max_frames, node_start = _layout(frame_counts, det_counts, dev)
    scores = torch.from_numpy(np.concatenate(mats) if mats else np.zeros(0)).to(dev)
    init = torch.from_numpy(np.concatenate(inits) if inits else np.zeros(0)).to(dev)
    return LinkResult(_ext.link_paths(scores, mat_off, init, det_off, frame_off, max_dets, max_frames, max_paths), node_start, max_paths)


def compute_link_scores(confs_a: np.ndarray, confs_b: np.ndarray, bboxes_a: np.ndarray, bboxes_b: np.ndarray,
                        tracks: np.ndarray, iou_thresh: float) -> np.ndarray:
    """(|A|, |B|) float64: c(a) + c(b) + [some track overlaps both by IoU > iou_thresh]."""
    return compute_score_seq([confs_a, confs_b], [bboxes_a, bboxes_b], [tracks], iou_thresh)[0]


def compute_score_seq(conf_seq: Sequence[np.ndarray], bbox_seq: Sequence[np.ndarray], track_seq: Sequence[np.ndarray],
                      iou_thresh: float) -> List[np.ndarray]:
    if len(conf_seq) != len(bbox_seq):
        raise ValueError(f"recieved |conf_seq|={len(conf_seq)}, but |bbox_seq|={len(bbox_seq)}")
    if len(track_seq) != len(conf_seq) - 1:
        raise ValueError(f"recieved |track_seq|={len(track_seq)} but |det_seq|={len(conf_seq)}")
    if len(conf_seq) < 2:
        return []
    scores, status, _, D = _score_problem(conf_seq, bbox_seq, track_seq, iou_thresh, paths=False)
    host = scores.cpu().numpy()
    out, o = [], 0
    for t in range(len(D) - 1):
        n = D[t] * D[t + 1]
        out.append(host[o:o + n].reshape(D[t], D[t + 1]))
        o += n
    return out


def _score_problem(conf_seq, bbox_seq, track_seq, iou_thresh, paths):
    confs = [_f32(c, "confidences").reshape(-1) for c in conf_seq]
    boxes = [_f32(b, "bounding boxes").reshape(-1, 4) for b in bbox_seq]
    tracks = [_f32(t, "tracks").reshape(-1, 4) for t in track_seq]
    D = [len(c) for c in confs]
    for c, b in zip(confs, boxes):
        if len(b) != len(c):
            raise ValueError(f"{len(c)} confidences but {len(b)} boxes")
    dev = _device()
    to = lambda parts, shape: torch.from_numpy(np.concatenate(parts).reshape(shape) if parts else np.zeros((0,) + shape[1:], np.float32)).to(dev)
    scores, status, result = link_batched(to(confs, (-1,)), to(boxes, (-1, 4)), to(tracks, (-1, 4)), D, [len(t) for t in tracks],
                                          [len(D)], iou_thresh, max_paths=0) if paths else (None, None, None)
    if not paths:
        det_off, frame_off, mat_off, M, max_dets, _, _ = _layout([len(D)], D, dev)
        tc = [len(t) for t in tracks]
        if max(tc, default=0) > _native.LINK_MAX_TRACKS:
            raise ValueError(f"at most {_native.LINK_MAX_TRACKS} tracks per frame pair, got {max(tc)}")
        track_off = torch.from_numpy(_offsets(tc).astype(np.int32)).to(dev)
        scores, status = _ext.link_scores(to(confs, (-1,)), to(boxes, (-1, 4)), det_off, frame_off, to(tracks, (-1, 4)), track_off,
                                          mat_off, iou_thresh, M, max_dets, max(tc, default=0))
    if int(status.item()) != _native.LINK_OK:
        raise RuntimeError(f"link scores failed with status {int(status.item())}")
    return scores, status, result, D


def viterbi(score_seq: List[np.ndarray], init_scores: Sequence[float] = None) -> Tuple[List[int], float]:
    if not score_seq and init_scores is None:
        raise ValueError("if no transitions init_scores need to be passed in.")
    (_, _), score, path = link_matrices_batched([(score_seq, init_scores)], max_paths=1).paths(0)[0]
    return path, score


def viterbi_multi_link(score_seq: List[np.ndarray], init_scores: List[float] = None) -> List[Tuple[Tuple[int, int], float, List[int]]]:
    if not score_seq and init_scores is None:
        raise ValueError("if no transitions, init_scores need to be passed in.")
    return link_matrices_batched([(score_seq, init_scores)], max_paths=0).paths(0)


def viterbi_tracking(conf_seq: List[np.ndarray], bbox_seq: List[np.ndarray], track_seq: List[np.ndarray], iou_thresh: float,
                     min_len: int) -> List[Tuple[Tuple[int, int], np.ndarray]]:
    if len(conf_seq) != len(bbox_seq):
        raise ValueError(f"recieved |conf_seq|={len(conf_seq)}, but |bbox_seq|={len(bbox_seq)}")
    if len(track_seq) != len(conf_seq) - 1:
        raise ValueError(f"recieved |track_seq|={len(track_seq)} but |det_seq|={len(conf_seq)}")
    if len(conf_seq) == 1 and len(conf_seq[0]) == 0:
        raise IndexError("list index out of range")                  # the reference: score_seq[0] of an empty sequence
    _, _, result, _ = _score_problem(conf_seq, bbox_seq, track_seq, iou_thresh, paths=True)
    tubelets = []
    for (start_ts, end_ts), _, track_path in result.paths(0):
        if end_ts - start_ts + 1 >= min_len:
            tubelets.append(((start_ts, end_ts),
                             np.array([bbox_seq[ts][node] for ts, node in zip(range(start_ts, end_ts + 1), track_path)])))
    return tubelets
