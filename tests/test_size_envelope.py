"""GPU: every tuned kernel at the edge of its own 32-bit offset guard, and one step past it.

The tuned kernels address memory with 32-bit byte offsets (buffer descriptors, int index arithmetic) and decide for themselves
whether they can take a call (the *_supported() predicates).  A wrapped offset in a buffer load does not fault -- the range check
returns 0 -- so an off-by-one in a predicate, or an int where an unsigned was needed, gives silently wrong numbers.  Each case here
runs just inside one predicate's bound (tensors of 2 to 4 GiB per batch item) and one step past it, where the next kernel of the
dispatch takes the call.

Each edge is computed from the predicate's own formula (file:line cited on the function), so a changed constant moves the test.
Which kernel ran is shown on each side by the demanded selector (impl = 2 succeeds inside, raises outside: the ABI refuses before
any launch) or by the workspace query, which changes design at the edge (tests/test_capi_symbols.py pins those transitions
without a GPU).

References stay cheap at these sizes: inputs are dense seeded random data made on the device (a wrapped read picks up wrong
NON-zero data); only what an independent small computation states exactly is compared -- probe channels of the backward against
the f64 oracle, the forward against the generic kernel on the probe channels / on RoI chunks, bit for bit.
"""
import gc

import numpy as np
import pytest
import torch

from conftest import ADVERSARIAL_ROIS, NEGATIVE_ROIS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GiB = 1 << 30
IMPL_AUTO, IMPL_GENERIC, IMPL_MFMA, IMPL_FAST = 0, 1, 2, 5
H0, W0 = 38, 63                         # the model's map
D, CELLS = 8, 17 * 17

# ---- the predicates' constants and edges (host arithmetic; tests/test_capi_symbols.py pins them through the workspace queries)
SG_KC = 16                              # d2t_corr_tuned.hip:104, channels per staged chunk
TP = 4                                  # d2t_corr_common.hpp:17, p-tile edge
LDS_MAX = 160 * 1024                    # d2t_pool_common.hpp:10
RD_CG, RD_GEO = 8, 32                   # d2t_roipool_fwd_direct.hip: channels per workgroup, geometry bytes per RoI
KK = 49


def corr_fwd_c_edge(H, W):
    """Largest C with (C + 8 SG_KC) H W 4 < 0x7ffffff0: corr_fwd_supported, d2t_corr_tuned.hip:587."""
    return (0x7ffffff0 - 1) // (H * W * 4) - 8 * SG_KC


def corr_bwd_c_edge(H, W):
    """Largest C with (C + 64) H W 4 + 64 W < 0x7ffffff0: corr_bwd8_supported, d2t_corr_bwd8.hip:491."""
    return (0x7ffffff0 - 1 - 64 * W) // (H * W * 4) - 64


def corr_bwd_h_edge():
    """Largest H with ceil(H / TP) <= 250: corr_bwd8_supported, d2t_corr_bwd8.hip:488."""
    return 250 * TP


def roipool_bwd_c_edge(R):
    """Largest C with R C 49 4 < 0xfffffff0: roipool_bwd_mfma_supported, d2t_pool_bwd.hip:532."""
    return (0xfffffff0 - 1) // (R * KK * 4)


def psroipool_bwd_r_edge(nT):
    """Largest R with R nT 49 4 < 0x7ffffff0: psroipool_bwd_rows_supported, d2t_pool_bwd.hip:1413."""
    return (0x7ffffff0 - 1) // (nT * KK * 4)


def roipool_fwd_direct_fits(R, C, H, W):
    """The direct k = 7 forward takes the call (roipool_fwd_direct_supported, d2t_roipool_fwd_direct.hip:196-201 through direct_plan):
    the planes leave LDS for the geometry of ceil(R / 65535) RoIs, and the output's element count fits int32."""
    return H <= 255 and W <= 255 and H * W * RD_CG * 4 + RD_GEO * -(-R // 65535) <= LDS_MAX and R * C * KK < 0x7fffffff


# ---- helpers
def _lib():
    from detect_to_track.models import _native
    return _native.lib


@pytest.fixture(autouse=True)
def _release_memory(request):
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    print(f"\n{request.node.nodeid}: peak {peak / GiB:.2f} GiB")
    gc.collect()
    torch.cuda.empty_cache()


def _require(nbytes):
    free, _ = torch.cuda.mem_get_info()
    short = nbytes + 2 * GiB - free
    if short > 0:
        pytest.skip(f"needs {nbytes / GiB:.1f} GiB + 2 GiB free on the device; short by {short / GiB:.1f} GiB")


def _gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def _probe_channels(C):
    """0, 1, 15, 16 (across the first 16-channel chunk), C / 2, every channel of the last 16-channel chunk, C - 1."""
    last = (C - 1) // 16 * 16
    return sorted({0, 1, 15, 16, C // 2, *range(last, C), C - 1})


def _same_bits(a, b, what):
    """Bit for bit, NaNs included (the kernels produce the same quiet NaN of 0 / 0)."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    ne = a.view(torch.int32) != b.view(torch.int32)
    n = int(ne.sum())
    assert n == 0, f"{what}: {n} of {a.numel()} elements differ in their bits (first at flat index {int(ne.flatten().nonzero()[0])})"


def _rois(R, seed, specials_at=()):
    """R boxes of BASELINE.md section 5 (centre U(0.15, 0.85)^2, size U(0.05, 0.6)^2), with the adversarial and negative boxes of
    tests/conftest.py written over the RoIs from each index of specials_at on."""
    g = _gen(seed)
    rois = torch.cat([0.15 + 0.7 * torch.rand(R, 2, generator=g, device=DEV),
                      0.05 + 0.55 * torch.rand(R, 2, generator=g, device=DEV)], 1)
    special = torch.tensor(ADVERSARIAL_ROIS + NEGATIVE_ROIS, dtype=torch.float32, device=DEV)
    for r in specials_at:
        r = max(0, min(r, R - len(special)))
        rois[r:r + len(special)] = special
    return rois.contiguous()


def _offset_rois(R, row_bytes):
    """First, last, and the RoIs whose output rows hold bytes 2^31 and 2^32 (when the output reaches that far)."""
    at = [0, R - 1]
    for edge in (1 << 31, 1 << 32):
        if R * row_bytes > edge:
            at += [edge // row_bytes - 1, edge // row_bytes]
    return at


# ---------------------------------------------------------------- correlation forward
@pytest.mark.parametrize("B, side", [(1, "inside"), (2, "inside"), (1, "past")],
                         ids=["B1-C_edge-corr_tuned.hip:587", "B2-C_edge-corr_tuned.hip:587", "B1-C_edge+1-blocked"])
def test_corr_fwd_offset_edge(B, side, oracle):
    """corr_fwd_supported (d2t_corr_tuned.hip:587): (C + 8 SG_KC) H W 4 < 0x7ffffff0 at 38 x 63 -- C = 224,128 inside (at B = 2 each map
    is 4 GiB, item 1 lies past 2^32), C = 224,129 one step past (the blocked kernel of d2t_corr_blocked.hip).  One map is dense, the
    other zero outside the probe channels: the exact-zero terms leave a sequential f32 sum unchanged, so the default dispatch equals
    the generic kernel on the packed probe channels bit for bit; D2T_IMPL_FAST is held to the 1e-5 contract.  Both orientations."""
    from detect_to_track.models import _ext
    H, W = H0, W0
    C = corr_fwd_c_edge(H, W) + (side == "past")
    _require(2 * B * C * H * W * 4)
    ws = _lib().d2t_corr_fwd_workspace_bytes(B, C, H, W, D, 1, 4)
    probe = _probe_channels(C)
    pidx = torch.tensor(probe, device=DEV)
    g = _gen(1000 + B)
    dense = torch.randn(B, C, H, W, generator=g, device=DEV)
    sparse = torch.zeros(B, C, H, W, device=DEV)
    sparse[:, pidx] = torch.randn(B, len(probe), H, W, generator=g, device=DEV)
    for orient, (fm0, fm1) in (("dense x sparse", (dense, sparse)), ("sparse x dense", (sparse, dense))):
        p0, p1 = fm0[:, pidx].contiguous(), fm1[:, pidx].contiguous()
        want = _ext.pointwise_correlation_forward(p0, p1, D, 1, IMPL_GENERIC)
        _same_bits(_ext.pointwise_correlation_forward(fm0, fm1, D, 1), want, f"default, {orient}, C = {C}")
        if side == "inside":
            _same_bits(_ext.pointwise_correlation_forward(fm0, fm1, D, 1, IMPL_MFMA), want, f"impl 2, {orient}, C = {C}")
            fast = _ext.pointwise_correlation_forward(fm0, fm1, D, 1, IMPL_FAST).cpu().numpy()
            a, b = p0.cpu().numpy(), p1.cpu().numpy()
            ref = oracle.corr_fwd(a.astype(np.float64), b.astype(np.float64), D, 1)
            mag = oracle.corr_fwd(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64), D, 1)
            oracle.assert_within_contract(fast, ref, mag, 1e-5, f"impl FAST, {orient}, C = {C}")
        else:
            with pytest.raises(RuntimeError):                       # refused before any launch: not the tuned kernels' shape
                _ext.pointwise_correlation_forward(fm0, fm1, D, 1, IMPL_MFMA)
    # witness of the design: the tuned forward's channel-split scratch inside, none for the blocked kernel past the edge
    assert (ws > 0) == (side == "inside"), ws


# ---------------------------------------------------------------- correlation backward
def _corr_bwd_check(oracle, B, C, H, W, side, seed):
    from detect_to_track.models import _ext
    g = _gen(seed)
    fm0 = torch.randn(B, C, H, W, generator=g, device=DEV)
    fm1 = torch.randn(B, C, H, W, generator=g, device=DEV)
    gout = torch.randn(B, H, W, 2 * D + 1, 2 * D + 1, generator=g, device=DEV)
    ws = _lib().d2t_corr_bwd_workspace_bytes(B, C, H, W, D, 1, 4)
    if side == "inside":
        assert ws == 0                                               # the strip kernel needs no scratch
        g0, g1 = _ext.pointwise_correlation_backward(gout, fm0, fm1, D, 1, IMPL_MFMA)   # demanded: the tuned kernel ran
    else:
        assert ws >= B * H * W * CELLS * 4                           # the blocked kernel's gradOut by displaced pixel
        with pytest.raises(RuntimeError):
            _ext.pointwise_correlation_backward(gout, fm0, fm1, D, 1, IMPL_MFMA)
        g0, g1 = _ext.pointwise_correlation_backward(gout, fm0, fm1, D, 1)
    probe = _probe_channels(C)
    pidx = torch.tensor(probe, device=DEV)
    (o0, o1), (m0, m1) = oracle.corr_bwd_acc64(gout.cpu().numpy(), fm0[:, pidx].cpu().numpy(), fm1[:, pidx].cpu().numpy(), D, 1)
    oracle.assert_within_contract(g0[:, pidx].cpu().numpy(), o0, m0, 1e-5, f"gradFM0, C = {C}, H = {H}, W = {W}")
    oracle.assert_within_contract(g1[:, pidx].cpu().numpy(), o1, m1, 1e-5, f"gradFM1, C = {C}, H = {H}, W = {W}")


@pytest.mark.parametrize("side", ["inside", "past"], ids=["C_edge-corr_bwd8.hip:491", "C_edge+1-blocked"])
def test_corr_bwd_offset_edge(side, oracle):
    """corr_bwd8_supported (d2t_corr_bwd8.hip:491): (C + 64) H W 4 + 64 W < 0x7ffffff0 at B = 1, 38 x 63 -- C = 224,192 inside (the strip
    kernel, demanded), C = 224,193 past (the blocked kernel with its 6 GB workspace: up to 15 GiB in all).  gradFM0[:, c] depends only on
    gradOut and FM1[:, c] (and likewise gradFM1): probe channels against the f64 oracle on the packed channels, within contract."""
    H, W = H0, W0
    C = corr_bwd_c_edge(H, W) + (side == "past")
    _require(4 * C * H * W * 4 + _lib().d2t_corr_bwd_workspace_bytes(1, C, H, W, D, 1, 4))
    _corr_bwd_check(oracle, 1, C, H, W, side, 2000)


@pytest.mark.parametrize("W", [20, 63])
@pytest.mark.parametrize("side", ["inside", "past"], ids=["H_edge-corr_bwd8.hip:488", "H_edge+1-blocked"])
def test_corr_bwd_row_tiles_edge(side, W, oracle):
    """corr_bwd8_supported (d2t_corr_bwd8.hip:488): ceil(H / 4) <= 250 (super-step numbers packed into 8 bits) -- H = 1000 inside, 1001
    past; a small, partial channel count (24), every channel checked."""
    C, H = 24, corr_bwd_h_edge() + (side == "past")
    _corr_bwd_check(oracle, 1, C, H, W, side, 3000 + W)


# ---------------------------------------------------------------- ROIPool backward
@pytest.mark.parametrize("side", ["inside", "past"], ids=["C_edge-pool_bwd.hip:532", "C_edge+1-pixel"])
def test_roipool_bwd_gemm_edge(side, oracle):
    """roipool_bwd_mfma_supported (d2t_pool_bwd.hip:532): gradOut below 0xfffffff0 bytes, read with a (unsigned) byte count -- R = 4000,
    C = 5478 (gradOut 4.0 GiB: every signed-offset slip shows) inside, C = 5479 past (the pixel form and its 4 GiB transposed copy, seen in
    the workspace query).  gradFM[c] depends only on gradOut[:, c]: probe channels against the f64 oracle, within contract."""
    from detect_to_track.models import _ext
    R, H, W = 4000, H0, W0
    C = roipool_bwd_c_edge(R) + (side == "past")
    ws = _lib().d2t_roipool_bwd_workspace_bytes(R, C, H, W, 7, 4)
    if side == "inside":
        assert ws < R * C * KK * 4                                   # the GEMM form: row lists only
    else:
        assert ws >= R * C * KK * 4                                  # the pixel form: gradOut transposed
    _require(R * C * KK * 4 + ws + C * H * W * 4)
    rois = _rois(R, 4000, _offset_rois(R, C * KK * 4))
    gout = torch.randn(R, C, 7, 7, generator=_gen(4001), device=DEV)
    gin = _ext.roipool_backward(gout, rois, H, W)
    pidx = torch.tensor(_probe_channels(C), device=DEV)
    want, mag = oracle.roipool_bwd_acc64(gout[:, pidx].cpu().numpy(), rois.cpu().numpy(), H, W)
    oracle.assert_within_contract(gin[pidx].cpu().numpy(), want, mag, 1e-5, f"ROIPool gradFM, R = {R}, C = {C}")


# ---------------------------------------------------------------- ROIPool forward (direct kernel)
ROIPOOL_FWD_CASES = [  # (R, C, H, W)
    (300, 1024, 20, 255),               # planes 163,200 B: room for the geometry of 20 RoIs -- 15 shares
    (300, 1024, 255, 20),
    (1_000_000, 8, 38, 63),             # 2,726 RoIs beside the planes: 367 shares
    (1_500_000, 16, 38, 63),            # output 4.7 GB: rows past 2^31 and 2^32
    (300, 1024, 21, 245),               # planes 164,640 B > 160 KiB: the summed-area kernel
]


@pytest.mark.parametrize("case", ROIPOOL_FWD_CASES, ids=lambda c: "R{}-C{}-{}x{}-{}".format(
    *c, "direct_fwd.hip:196" if roipool_fwd_direct_fits(*c) else "past-LDS-summed_area"))
def test_roipool_fwd_direct_lds_edge(case):
    """roipool_fwd_direct_supported (d2t_roipool_fwd_direct.hip:196, direct_plan): the direct k = 7 kernel takes every map whose 8
    interleaved planes leave LDS for ceil(R / 65535) RoIs' geometry, whatever R -- its result (default and demanded) is then the generic
    kernel's, bit for bit, NaN pattern included.  Past the LDS the summed-area kernel answers: 1e-5, NaN pattern exact.  Outputs are
    independent per RoI: the generic kernel runs on chunks of the RoI list, adversarial and negative boxes sit where the output crosses
    2^31 / 2^32 bytes."""
    from detect_to_track.models import _ext
    R, C, H, W = case
    direct = roipool_fwd_direct_fits(R, C, H, W)
    out_bytes = R * C * KK * 4
    chunk = max(1, (256 << 20) // (C * KK * 4))
    _require(out_bytes + 2 * chunk * C * KK * 4 + C * H * W * 4)
    fm = torch.randn(C, H, W, generator=_gen(5000 + R), device=DEV)
    rois = _rois(R, 5001, _offset_rois(R, C * KK * 4))
    for impl in ((IMPL_AUTO, IMPL_MFMA) if direct else (IMPL_AUTO,)):
        out = _ext.roipool_forward(fm, rois, 7, impl)
        for r0 in range(0, R, chunk):
            got = out[r0:r0 + chunk]
            want = _ext.roipool_forward(fm, rois[r0:r0 + chunk].contiguous(), 7, IMPL_GENERIC)
            if direct:
                _same_bits(got, want, f"impl {impl}, RoIs {r0}..")
            else:
                assert torch.equal(torch.isnan(got), torch.isnan(want)), f"NaN pattern, RoIs {r0}.."
                torch.testing.assert_close(torch.nan_to_num(got), torch.nan_to_num(want), rtol=1e-5, atol=1e-5)
        del out


# ---------------------------------------------------------------- PSROIPool at the rows design's edge
@pytest.mark.parametrize("side", ["inside", "past"], ids=["R_edge-pool_bwd.hip:1413", "R_edge+1-next_design"])
def test_psroipool_bwd_rows_edge(side, oracle):
    """psroipool_bwd_rows_supported (d2t_pool_bwd.hip:1413): R nT 49 4 < 0x7ffffff0 -- nT = 32, R = 342,392 inside (gradOut 2 GiB), 342,393
    past (rows and GEMM both out; the workspace query changes design).  Every gradFM channel against the f64 oracle, within contract."""
    from detect_to_track.models import _ext
    nT, H, W = 32, H0, W0
    R = psroipool_bwd_r_edge(nT) + (side == "past")
    ws = _lib().d2t_psroipool_bwd_workspace_bytes(R, nT, H, W, 7, 4)
    other = _lib().d2t_psroipool_bwd_workspace_bytes(R - 1 if side == "past" else R + 1, nT, H, W, 7, 4)
    assert ws != other                                               # one side of the edge is the rows design, the other is not
    _require(R * nT * KK * 4 + ws + nT * KK * H * W * 4)
    rois = _rois(R, 6000, _offset_rois(R, nT * KK * 4))
    gout = torch.randn(R, nT, 7, 7, generator=_gen(6001), device=DEV)
    gin = _ext.ps_roipool_backward(gout, rois, H, W)
    # (gradFM channels are shared between targets -- the reference's channel (t + 1) (i k + j), oracle/d2t_oracle_impl.h -- so every
    # channel is checked, against the oracle on the whole gradOut)
    want, mag = oracle.psroipool_bwd_acc64(gout.cpu().numpy(), rois.cpu().numpy(), H, W)
    oracle.assert_within_contract(gin.cpu().numpy(), want, mag, 1e-5, f"PSROIPool gradFM, R = {R}")


def test_psroipool_fwd_at_rows_edge():
    """The PSROIPool forward (psroipool_fwd_supported, d2t_pool_tuned.hip:697) at the same R, nT: output 2 GiB, every RoI against the
    generic kernel on chunks of the RoI list, bit for bit."""
    from detect_to_track.models import _ext
    nT, H, W = 32, H0, W0
    R = psroipool_bwd_r_edge(nT)
    chunk = 20_000
    _require(R * nT * KK * 4 + 2 * chunk * nT * KK * 4)
    fm = torch.randn(nT * KK, H, W, generator=_gen(7000), device=DEV)
    rois = _rois(R, 7001, _offset_rois(R, nT * KK * 4))
    out = _ext.ps_roipool_forward(fm, rois, nT, 7)
    for r0 in range(0, R, chunk):
        want = _ext.ps_roipool_forward(fm, rois[r0:r0 + chunk].contiguous(), nT, 7, IMPL_GENERIC)
        _same_bits(out[r0:r0 + chunk], want, f"RoIs {r0}..")
