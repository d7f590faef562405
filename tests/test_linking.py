"""Tubelet linking (reference detect_to_track/viterbi.py) on the device: csrc/d2t_link.hip through the C ABI, the torch wrappers
and detect_to_track/viterbi.py, against the reference's own outputs (tests/golden/link_*.npz, make_link_golden.py) and the
numpy restatement of the contract (tests/link_reference.py).  Every comparison is exact: paths, their order, score bits."""
import time

import numpy as np
import pytest

import link_reference as L
from conftest import GOLDEN, load_golden

inf = np.inf
LINK_FIXTURES = sorted(GOLDEN.glob("link_*.npz"))


def _fixture(path):
    z = load_golden(path)
    D = [int(d) for d in z["D"]]
    flat = z["mats"].view(np.float64)
    mats, o = [], 0
    for t in range(len(D) - 1):
        n = D[t] * D[t + 1]
        mats.append(flat[o:o + n].reshape(D[t], D[t + 1]).copy())
        o += n
    z["mats_list"] = mats
    po = np.concatenate([[0], np.cumsum(z["p_len"])])
    z["paths"] = [((int(z["p_start"][k]), int(z["p_end"][k])), int(z["p_score"][k]), [int(v) for v in z["p_nodes"][po[k]:po[k + 1]]])
                  for k in range(len(z["p_len"]))]
    if str(z["kind"]) == "tracking":
        off, toff = np.concatenate([[0], np.cumsum(D)]), np.concatenate([[0], np.cumsum(z["n_tracks"])])
        z["conf_seq"] = [z["confs"][off[t]:off[t + 1]] for t in range(len(D))]
        z["bbox_seq"] = [z["boxes"][off[t]:off[t + 1]] for t in range(len(D))]
        z["track_seq"] = [z["tracks"][toff[t]:toff[t + 1]] for t in range(len(D) - 1)]
        z["init_arg"] = z["conf_seq"][0].tolist()
    else:
        z["init_arg"] = z["init"].tolist() if int(z["has_init"]) else None
    return z


def _bits(paths):
    return [(se, int(np.float64(s).view(np.uint64)), list(p)) for se, s, p in paths]


# ------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("path", LINK_FIXTURES, ids=[p.stem for p in LINK_FIXTURES])
def test_restatement_reproduces_reference_fixture(path):
    z = _fixture(path)
    if str(z["kind"]) == "tracking":
        mats = [L.link_scores(z["conf_seq"][t], z["conf_seq"][t + 1], z["bbox_seq"][t], z["bbox_seq"][t + 1], z["track_seq"][t],
                              float(z["iou_thresh"])) for t in range(len(z["D"]) - 1)]
        for got, want in zip(mats, z["mats_list"]):
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        assert len(L.tracking(z["conf_seq"], z["bbox_seq"], z["track_seq"], float(z["iou_thresh"]), int(z["min_len"]))) == int(z["n_tubelets"])
    got = L.multi_link(z["mats_list"], z["init_arg"], 1 if str(z["kind"]) == "viterbi" else 0)
    assert _bits(got) == z["paths"]


def test_fixtures_cover_the_contract():
    kinds = {p.stem: str(np.load(p)["kind"]) for p in LINK_FIXTURES}
    for name in ("link_single_frame", "link_empty_frames", "link_conf_ties", "link_restarts", "link_neginf_masks", "link_viterbi_init"):
        assert name in kinds, name
    assert sum(k == "tracking" for k in kinds.values()) >= 6 and "viterbi" in kinds.values()


def test_restatement_known_answer():
    mats = [np.array([[0.3, -inf], [0.2, 0.4]]), np.array([[-inf, 0.1], [0.5, 0.2]])]
    keep = [m.copy() for m in mats]
    assert L.multi_link(mats, [0.1, 0.2]) == [((0, 2), 1.1, [1, 1, 0]), ((0, 2), 0.5, [0, 0, 1])]
    assert all(np.array_equal(a, b) for a, b in zip(mats, keep))


def test_restatement_flags_non_termination():
    with pytest.raises(L.NonTermination):
        L.multi_link([np.zeros((2, 2))], [0.0, 0.0])


@pytest.fixture(scope="module")
def native():
    from detect_to_track.models import _native
    return _native


def test_version_109(native):
    assert native.version() >= 109                    # 1.09: tubelet linking (d2t_link_*)


def test_link_argument_validation_without_device(native):
    L_ = native.lib
    EINVAL, ETOOBIG, EWS = -1, -2, -3
    P8 = 0x1000                                        # never dereferenced: every call below fails its host checks
    ws = L_.d2t_link_workspace_bytes(100, 100)
    assert ws >= 2 * 100 * 2 * 8 and ws >= 100 * 13
    assert L_.d2t_link_workspace_bytes(-1, 0) == 0
    # (confs, boxes, det_off, frame_off, tracks, track_off, mat_off, thr, P, F, N, NT, M, max_dets, max_tracks, scores, status, ws, ws_bytes, stream)
    ok = [P8, P8, P8, P8, P8, P8, P8, 0.5, 2, 5, 40, 10, 300, 10, 5, P8, P8, P8, ws, None]

    def scores(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{"confs": 0, "boxes": 1, "det_off": 2, "tracks": 4, "P": 8, "F": 9, "N": 10, "NT": 11, "M": 12, "max_dets": 13,
               "max_tracks": 14, "scores": 15, "status": 16, "ws": 17, "ws_bytes": 18}[k]] = v
        return L_.d2t_link_scores_f32(*a)
    assert scores(max_dets=1025) == ETOOBIG
    assert scores(max_tracks=1025) == ETOOBIG
    assert scores(P=-1) == EINVAL and scores(N=-1) == EINVAL and scores(F=1) == EINVAL
    assert scores(confs=None) == EINVAL and scores(status=None) == EINVAL and scores(scores=None) == EINVAL
    assert scores(det_off=None) == EINVAL
    assert scores(boxes=P8 + 4) == EINVAL and scores(ws=P8 + 8) == EINVAL
    assert scores(ws=None) == EWS and scores(ws_bytes=16) == EWS
    # (scores, mat_off, init, det_off, frame_off, P, F, N, M, max_dets, max_frames, max_paths, start, len, score, nodes, count, status, ws, ws_bytes, stream)
    ok = [P8, P8, P8, P8, P8, 2, 5, 40, 300, 10, 3, 0, P8, P8, P8, P8, P8, P8, P8, ws, None]

    def paths(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[{"scores": 0, "mat_off": 1, "det_off": 3, "P": 5, "F": 6, "N": 7, "M": 8, "max_dets": 9, "max_frames": 10,
               "max_paths": 11, "start": 12, "nodes": 15, "count": 16, "status": 17, "ws": 18, "ws_bytes": 19}[k]] = v
        return L_.d2t_link_paths_f64(*a)
    assert paths(max_dets=1025) == ETOOBIG and paths(max_frames=8193) == ETOOBIG
    assert paths(max_paths=2) == EINVAL and paths(max_paths=-1) == EINVAL
    assert paths(F=1) == EINVAL and paths(M=-1) == EINVAL
    assert paths(scores=None) == EINVAL and paths(mat_off=None) == EINVAL and paths(det_off=None) == EINVAL
    assert paths(start=None) == EINVAL and paths(nodes=None) == EINVAL and paths(count=None) == EINVAL and paths(status=None) == EINVAL
    assert paths(ws=P8 + 4) == EINVAL
    assert paths(ws=None) == EWS and paths(ws_bytes=100) == EWS
    assert paths(P=0) == 0                               # nothing to do: no launch


def test_python_surface_raises_like_the_reference():
    from detect_to_track import viterbi as V
    c, b = np.ones(2, np.float32), np.zeros((2, 4), np.float32)
    with pytest.raises(ValueError):
        V.compute_score_seq([c, c], [b], [b], 0.5)
    with pytest.raises(ValueError):
        V.compute_score_seq([c, c], [b, b], [], 0.5)
    with pytest.raises(ValueError):
        V.viterbi([], None)
    with pytest.raises(ValueError):
        V.viterbi_multi_link([], None)
    with pytest.raises(IndexError):
        V.viterbi_tracking([np.zeros(0, np.float32)], [np.zeros((0, 4), np.float32)], [], 0.5, 1)
    with pytest.raises(TypeError):
        V.compute_link_scores(c.astype(np.float64), c, b, b, b, 0.5)
    with pytest.raises(TypeError):
        V.viterbi_multi_link([np.zeros((2, 2), np.float32)], None)


# ------------------------------------------------------------------------------------------------------------ GPU
def _random_tracking(rng, T, dmax, ntr_max=None):
    D = [int(rng.integers(0, dmax + 1)) for _ in range(T)]
    confs = [rng.random(d).astype(np.float32) for d in D]
    boxes = [np.concatenate([rng.uniform(0.2, 0.8, (d, 2)), rng.uniform(0.05, 0.5, (d, 2))], 1).astype(np.float32) for d in D]
    tracks = []
    for t in range(T - 1):
        hi = D[t] if ntr_max is None else min(D[t], ntr_max)
        n = int(rng.integers(0, hi + 1))
        base = boxes[t][rng.integers(0, D[t], n)] if D[t] else np.zeros((n, 4), np.float32)
        tr = base + rng.normal(0, 0.04, (n, 4)).astype(np.float32)
        tr[:, 2:] = np.abs(tr[:, 2:])
        tracks.append(tr.astype(np.float32).reshape(-1, 4))
    return confs, boxes, tracks


def _reference_or_flag(mats, init, max_paths=0):
    try:
        return L.multi_link(mats, init, max_paths)
    except L.NonTermination:
        return "nonterminating"


def _device_or_flag(result, p):
    try:
        return result.paths(p)
    except RuntimeError:
        return "nonterminating"


def _problems(seed):
    """>= 200 seeded problems: T 1..128, D 0..1024 (the limit included), tracks 0..D, iou 0.3 / 0.5 / 0.7.  Sizes are bounded so
    that the numpy restatement stays fast: long sequences have few detections, the widest frames come in short sequences."""
    rng = np.random.default_rng(seed)
    shapes = ([(int(rng.integers(1, 129)), int(rng.integers(0, 9))) for _ in range(120)] +
              [(int(rng.integers(1, 33)), int(rng.integers(8, 65))) for _ in range(70)] +
              [(int(rng.integers(2, 6)), int(rng.integers(64, 257))) for _ in range(12)] +
              [(2, 1024), (3, 1024), (2, 1000)])
    return [(T, d, [0.3, 0.5, 0.7][i % 3]) for i, (T, d) in enumerate(shapes)], rng


def _batch_tracking(problems, dev):
    import torch
    confs, boxes, tracks, D, TC, FC = [], [], [], [], [], []
    for c, b, t, _ in problems:
        confs += c; boxes += b; tracks += t
        D += [len(x) for x in c]; TC += [len(x) for x in t]; FC.append(len(c))
    cat = lambda xs, shape: torch.from_numpy(np.concatenate(xs).reshape(shape) if xs else np.zeros((0,) + shape[1:], np.float32)).to(dev)
    return cat(confs, (-1,)), cat(boxes, (-1, 4)), cat(tracks, (-1, 4)), D, TC, FC


@pytest.mark.gpu
@pytest.mark.parametrize("path", LINK_FIXTURES, ids=[p.stem for p in LINK_FIXTURES])
def test_device_reproduces_reference_fixture(path):
    from detect_to_track import viterbi as V
    z = _fixture(path)
    kind = str(z["kind"])
    if kind == "tracking":
        args = (z["conf_seq"], z["bbox_seq"], z["track_seq"], float(z["iou_thresh"]))
        got_mats = V.compute_score_seq(*args)
        assert len(got_mats) == len(z["mats_list"])
        for got, want in zip(got_mats, z["mats_list"]):
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
        tubes = V.viterbi_tracking(*args, int(z["min_len"]))
        want_tubes = L.tracking(*args, int(z["min_len"]))
        assert len(tubes) == int(z["n_tubelets"]) == len(want_tubes)
        for (se, bx), (wse, wbx) in zip(tubes, want_tubes):
            assert se == wse and np.array_equal(bx, wbx)
        for t in range(len(z["D"]) - 1):                             # compute_link_scores, pair by pair
            got = V.compute_link_scores(z["conf_seq"][t], z["conf_seq"][t + 1], z["bbox_seq"][t], z["bbox_seq"][t + 1],
                                        z["track_seq"][t], float(z["iou_thresh"]))
            np.testing.assert_array_equal(got.view(np.uint64), z["mats_list"][t].view(np.uint64))
    keep = [m.copy() for m in z["mats_list"]]
    if kind == "viterbi":
        path_, score = V.viterbi(z["mats_list"], z["init_arg"])
        ((s, e), ws, wp), = z["paths"]
        assert path_ == wp and int(np.float64(score).view(np.uint64)) == ws
    else:
        assert _bits(V.viterbi_multi_link(z["mats_list"], z["init_arg"])) == z["paths"]
    assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(keep, z["mats_list"]))


@pytest.mark.gpu
def test_device_known_answer_and_non_termination():
    from detect_to_track import viterbi as V
    mats = [np.array([[0.3, -inf], [0.2, 0.4]]), np.array([[-inf, 0.1], [0.5, 0.2]])]
    assert V.viterbi_multi_link(mats, [0.1, 0.2]) == [((0, 2), 1.1, [1, 1, 0]), ((0, 2), 0.5, [0, 0, 1])]
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError):
        V.viterbi_multi_link([np.zeros((2, 2))], [0.0, 0.0])        # the reference never returns from this
    assert time.perf_counter() - t0 < 30.0


@pytest.mark.gpu
def test_device_matches_restatement_on_seeded_problems():
    """All problems in ONE call of each entry point (tracking flow), then the same matrices with extra -inf links straight into
    viterbi_multi_link's batched form; every problem against the restatement, scores and paths exact."""
    import torch
    from detect_to_track import viterbi as V
    shapes, rng = _problems(7)
    assert len(shapes) >= 200
    problems = []
    for T, dmax, iou in shapes:
        c, b, t = _random_tracking(rng, T, dmax)
        if dmax >= 1000:                                             # the limit itself, in every frame
            c = [rng.random(1024 if dmax == 1024 else 1000).astype(np.float32) for _ in range(T)]
            b = [np.concatenate([rng.uniform(0.2, 0.8, (len(x), 2)), rng.uniform(0.05, 0.5, (len(x), 2))], 1).astype(np.float32) for x in c]
            t = [(b[i][rng.integers(0, len(b[i]), 1024 if i == 0 else 300)] + np.float32(0.01)).astype(np.float32) for i in range(T - 1)]
        problems.append((c, b, t, iou))
    dev = torch.device("cuda", 0)
    # one iou threshold per call: group the problems by threshold
    for iou in (0.3, 0.5, 0.7):
        group = [pr for pr in problems if pr[3] == iou]
        scores, status, result = V.link_batched(*_batch_tracking(group, dev), iou)
        assert int(status.item()) == 0
        host = scores.cpu().numpy()
        o, masked = 0, []
        for p, (c, b, t, _) in enumerate(group):
            mats = []
            for k in range(len(c) - 1):
                want = L.link_scores(c[k], c[k + 1], b[k], b[k + 1], t[k], iou)
                got = host[o:o + want.size].reshape(want.shape)
                o += want.size
                np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
                mats.append(want)
            assert _device_or_flag(result, p) == _reference_or_flag(mats, c[0].astype(np.float64)), f"problem {p} (iou {iou})"
            m2 = [np.where(rng.random(m.shape) < 0.3, -inf, m) for m in mats]   # caller masks on top
            masked.append((m2, c[0].astype(np.float64).tolist() if len(c[0]) else None))
        masked = [(m, i) for m, i in masked if m or i]
        res = V.link_matrices_batched(masked)
        for p, (m, i) in enumerate(masked):
            assert _device_or_flag(res, p) == _reference_or_flag(m, i), f"masked problem {p} (iou {iou})"
        one = V.link_matrices_batched([(m, i) for m, i in masked if (m and m[-1].shape[1]) or (not m and i)], max_paths=1)
        for p, (m, i) in enumerate([(m, i) for m, i in masked if (m and m[-1].shape[1]) or (not m and i)]):
            assert one.paths(p) == L.multi_link(m, i, 1), f"viterbi problem {p} (iou {iou})"


@pytest.mark.gpu
def test_batched_equals_single_calls():
    import torch
    from detect_to_track import viterbi as V
    rng = np.random.default_rng(64)
    dev = torch.device("cuda", 0)
    problems = []
    for i in range(64):
        T, dmax = [(1, 6), (2, 40), (12, 12), (40, 5), (5, 90), (3, 0)][i % 6]
        c, b, t = _random_tracking(rng, T, dmax)
        problems.append((c, b, t, 0.5))
    scores, status, batch = V.link_batched(*_batch_tracking(problems, dev), 0.5)
    bscores = scores.cpu().numpy()
    o = 0
    for p, pr in enumerate(problems):
        s1, st1, single = V.link_batched(*_batch_tracking([pr], dev), 0.5)
        n = s1.numel()
        np.testing.assert_array_equal(bscores[o:o + n].view(np.uint64), s1.cpu().numpy().view(np.uint64))
        o += n
        assert _bits(_device_or_flag_list(batch, p)) == _bits(_device_or_flag_list(single, 0))


def _device_or_flag_list(result, p):
    r = _device_or_flag(result, p)
    return [] if r == "nonterminating" else r


@pytest.mark.gpu
def test_bad_layout_is_reported_not_followed():
    """Offsets that point outside the declared extents: the kernels check them before use and report, writing nothing."""
    import torch
    from detect_to_track.models import _ext, _native
    dev = torch.device("cuda", 0)
    det_off = torch.tensor([0, 3, 5000], dtype=torch.int32, device=dev)      # frame 1 claims nodes far beyond N = 6
    frame_off = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    mat_off = torch.tensor([0], dtype=torch.int64, device=dev)
    init = torch.zeros(6, dtype=torch.float64, device=dev)
    scores = torch.zeros(9, dtype=torch.float64, device=dev)
    out = _ext.link_paths(scores, mat_off, init, det_off, frame_off, 16, 2, 0)
    assert int(out[5].item()) == _native.LINK_BAD_LAYOUT and int(out[4].item()) == 0
    confs, boxes = torch.zeros(6, device=dev), torch.zeros((6, 4), device=dev)
    track_off = torch.tensor([0, 0], dtype=torch.int32, device=dev)
    _, st = _ext.link_scores(confs, boxes, det_off, frame_off, torch.zeros((0, 4), device=dev), track_off, mat_off, 0.5, 9, 16, 0)
    assert int(st.item()) == _native.LINK_BAD_LAYOUT
