"""numpy restatement of Viterbi tubelet linking (TEST INFRASTRUCTURE: imported by tests/ and tools/ only).

The contract (include/d2t_ops.h, linking section) in executable form, written as the device runs it: removal is a
per-node mask, never a write into the caller's matrices; after an extraction that starts at frame s only frames
max(s, 1).. are revisited, and there only the nodes whose own best source changed or was removed.

  link_scores(confs_a, confs_b, boxes_a, boxes_b, tracks, thr)   (|A|, |B|) float64
      s[a, b] = float64(float32(c_a + c_b)) + (1.0 if some track t has IoU(a, t) > thr and IoU(b, t) > thr else 0.0),
      IoU in float32 by oracle/regions.py:iou_one_to_many, thr rounded to float32.
  multi_link(mats, init, max_paths=0) -> [((start, end), score, [node, ...]), ...]
      max_paths = 0: every tubelet, in extraction order; max_paths = 1: the single best path (Viterbi).
      Raises NonTermination where repeated extraction would pick an already removed node forever.
"""
import numpy as np

from regions import iou_one_to_many


class NonTermination(RuntimeError):
    """The best final node of an extraction is one that an earlier extraction removed: the extraction would repeat forever."""


def match_bits(boxes, tracks, thr):
    """(|boxes|, |tracks|) bool: IoU(box, track) > thr, float32."""
    boxes, tracks = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(tracks, np.float32).reshape(-1, 4)
    out = np.zeros((len(boxes), len(tracks)), bool)
    if len(tracks):
        for i, b in enumerate(boxes):
            out[i] = iou_one_to_many(b, tracks) > np.float32(thr)
    return out


def link_scores(confs_a, confs_b, boxes_a, boxes_b, tracks, thr):
    ca, cb = np.asarray(confs_a, np.float32), np.asarray(confs_b, np.float32)
    ma, mb = match_bits(boxes_a, tracks, thr), match_bits(boxes_b, tracks, thr)
    psi = (ma.astype(np.uint8) @ mb.T.astype(np.uint8)) > 0 if ma.shape[1] else np.zeros((len(ca), len(cb)), bool)
    return (ca[:, None] + cb[None, :]).astype(np.float64) + np.where(psi, 1.0, 0.0)


def _best_sources(v_src, live_src, col):
    """For the columns `col` (|A|, k) of one transition matrix: (value, source) of every destination as the scan
    `best = 0.0; for a ascending: if v[a] + s[a, b] > best: take it` leaves them; removed sources never take part."""
    with np.errstate(invalid="ignore"):
        cand = v_src[:, None] + col
    ok = live_src[:, None] & (cand > 0.0)                                # NaN and -inf never win; 0.0 is the restart
    cand = np.where(ok, cand, -np.inf)
    if cand.shape[0] == 0:
        return np.zeros(cand.shape[1]), np.full(cand.shape[1], -1, np.int64)
    src = np.argmax(cand, axis=0)                                        # the first maximum
    val = cand[src, np.arange(cand.shape[1])]
    hit = ok[src, np.arange(cand.shape[1])]
    return np.where(hit, val, 0.0), np.where(hit, src, -1)


def multi_link(mats, init=None, max_paths=0):
    mats = [np.asarray(m, np.float64) for m in mats]
    T = len(mats) + 1
    if init is None:
        init = np.zeros(mats[0].shape[0]) if mats else np.zeros(0)
    init = np.asarray(init, np.float64)
    D = [len(init)] + [m.shape[1] for m in mats]
    for t, m in enumerate(mats):
        assert m.shape == (D[t], D[t + 1]), (t, m.shape, D)
    removed = [np.zeros(d, bool) for d in D]
    val = [init.copy()] + [np.zeros(d) for d in D[1:]]
    bp = [np.full(d, -1, np.int64) for d in D]
    for t in range(1, T):                                                # the full pass, once
        val[t], bp[t] = _best_sources(val[t - 1], ~removed[t - 1], mats[t - 1])

    def extract(final):
        node, path = None, []
        v = val[final]
        if final == 0:                                                   # Python's max(): first element, replaced only by a greater one
            for i in range(len(v)):
                if node is None or v[i] > v[node]:
                    node = i
        else:
            node = int(np.argmax(v))                                     # values >= 0.0, never NaN: the first maximum
        score = float(v[node])
        t = final
        while node >= 0:
            path.append(int(node))
            node = bp[t][node]
            t -= 1
        return (t + 1, final), score, path[::-1]

    if max_paths == 1:
        if D[T - 1] == 0:
            raise ValueError("max() arg is an empty sequence")
        return [extract(T - 1)]

    out = []
    for final in range(T - 1, 0, -1):
        m = mats[final - 1]
        fin = np.isfinite(m) & ~removed[final - 1][:, None] & ~removed[final][None, :]
        cnt = fin.sum(axis=0)                                            # finite live links into each live final node
        total = int(cnt.sum())
        guard = sum(D)
        while total > 0:
            (start, _), score, path = extract(final)
            if removed[final][path[-1]]:
                raise NonTermination(f"extraction at frame {final} picks removed node {path[-1]}")
            out.append(((start, final), score, path))
            guard -= 1
            assert guard >= 0
            for t, node in zip(range(start, final + 1), path):
                removed[t][node] = True
            total -= int(cnt[path[-1]])
            cnt[path[-1]] = 0
            if len(path) > 1:
                row = fin[path[-2]] & ~removed[final]
                cnt[row] -= 1
                total -= int(row.sum())
                fin[path[-2]] = False
            # revisit frames max(start, 1)..final: a node changes iff it was removed or its best source changed / went
            stale = np.zeros(D[max(start, 1) - 1], bool)
            if start == 0:
                stale[path[0]] = True
            for t in range(max(start, 1), final + 1):
                b_src = bp[t]
                dirty = removed[t].copy()
                if len(stale):
                    dirty |= (b_src >= 0) & stale[np.maximum(b_src, 0)]
                idx = np.nonzero(dirty & ~removed[t])[0]
                old = val[t].copy()
                val[t][removed[t]], bp[t][removed[t]] = 0.0, -1
                if len(idx):
                    val[t][idx], bp[t][idx] = _best_sources(val[t - 1], ~removed[t - 1], mats[t - 1][:, idx])
                stale = removed[t] | (val[t] != old)
    for node in range(D[0]):
        if not removed[0][node] and np.isfinite(init[node]):
            out.append(((0, 0), float(init[node]), [node]))
    return out


def tracking(conf_seq, bbox_seq, track_seq, iou_thresh, min_len):
    """viterbi_tracking: link scores, every tubelet, the boxes of those at least min_len frames long."""
    mats = [link_scores(conf_seq[t], conf_seq[t + 1], bbox_seq[t], bbox_seq[t + 1], track_seq[t], iou_thresh)
            for t in range(len(conf_seq) - 1)]
    paths = multi_link(mats, np.asarray(conf_seq[0], np.float32).astype(np.float64))
    return [((s, e), np.array([bbox_seq[t][n] for t, n in zip(range(s, e + 1), p)]))
            for (s, e), _, p in paths if e - s + 1 >= min_len]
