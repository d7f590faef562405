// d2t_link.hip -- Viterbi tubelet linking on the device: link scores between adjacent frames and repeated best-path
// extraction, for many independent (video, class) problems per launch.
//
// The reference does this on the host in pure Python (detect_to_track/viterbi.py: compute_link_scores :11,
// compute_score_seq :45, viterbi :71, viterbi_multi_link :119, viterbi_tracking :162).  The contract is the reference's
// result bit for bit (include/d2t_ops.h, linking section; tests/link_reference.py restates it):
//
//   link score   s[a][b] = (double)(float)(c_a + c_b) + (psi ? 1.0 : 0.0), psi = some track t with IoU(a, t) > thr and
//                IoU(b, t) > thr (float32 IoU, d2t_iou.hpp; thr rounded to float32)
//   viterbi      v[dst] = the first source (ascending) whose v[src] + s[src][dst] is strictly greater than the running best,
//                which starts at 0.0 with no source (a restart: the path begins at dst); the winner of the last frame is
//                the first maximum
//   multi-link   from the last frame down to frame 1: while the matrix into that frame has a finite live entry, extract the
//                best path ending there and remove its nodes; then every live frame-0 node with a finite init score is a
//                one-node path.  Removal is a per-node flag: the caller's matrices are never written.
//
// Ragged layout: problem p owns frames [frame_off[p], frame_off[p+1]); frame f owns nodes [det_off[f], det_off[f+1]);
// the pair (frame_off[p] + t, frame_off[p] + t + 1) is pair g = frame_off[p] - p + t, with tracks [track_off[g],
// track_off[g+1]) and its (D_a, D_b) matrix at scores + mat_off[g].  Every offset is read from device memory and checked
// against the extents the host validated before it is used: a layout that does not fit sets a status and writes nothing.
#include "d2t_kernels.hpp"
#include "d2t_iou.hpp"

namespace d2t {

namespace {

constexpr int LK_T = 1024;                    // threads of the per-problem path kernel (16 waves)
constexpr int LK_WAVES = LK_T / 64;
constexpr int LK_MAXD = D2T_LINK_MAX_DETS;     // detections per frame
constexpr int LK_MAXF = D2T_LINK_MAX_FRAMES;   // frames per problem (their node offsets are kept in LDS)
constexpr int LK_MAXTR = D2T_LINK_MAX_TRACKS;  // tracks per frame pair
constexpr int LK_ROWS = 16;                    // matrix rows per workgroup of the score kernel
constexpr int LK_ST = 256;                     // threads of the two score kernels

inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
inline int words_of(int max_tracks) { return max_tracks > 64 ? (max_tracks + 63) / 64 : 1; }

// The frames and node ranges of pair g, every offset checked against the validated extents.
struct Pair { int fa, na, nb, Da, Db, t0, ntr; long long m0; };

__device__ __forceinline__ bool pair_of(int g, const int* __restrict__ det_off, const int* __restrict__ frame_off,
                                        const int* __restrict__ track_off, const long long* __restrict__ mat_off,
                                        int P, int F, int N, int NT, long long M, int max_dets, int max_tracks, Pair& q)
{
    int lo = 0, hi = P - 1;                                          // the last problem whose first pair is <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_off[mid] - mid <= g) lo = mid; else hi = mid - 1;
    }
    const int f0 = frame_off[lo], f1 = frame_off[lo + 1];
    const int t = g - (f0 - lo);
    if (f0 < 0 || f1 > F || f1 - f0 < 1 || t < 0 || t >= f1 - f0 - 1) return false;
    q.fa = f0 + t;
    const int a0 = det_off[q.fa], a1 = det_off[q.fa + 1], b1 = det_off[q.fa + 2];
    if (a0 < 0 || a1 < a0 || b1 < a1 || b1 > N || a1 - a0 > max_dets || b1 - a1 > max_dets) return false;
    const int t0 = track_off[g], t1 = track_off[g + 1];
    if (t0 < 0 || t1 < t0 || t1 > NT || t1 - t0 > max_tracks) return false;
    q.na = a0; q.nb = a1; q.Da = a1 - a0; q.Db = b1 - a1; q.t0 = t0; q.ntr = t1 - t0;
    q.m0 = mat_off[g];
    return q.m0 >= 0 && q.m0 + (long long)q.Da * q.Db <= M;
}

// Match bitsets: word w of side s of node n = bits IoU(box_n, track 64w + j) > thr over the tracks of the pair in which n is
// the source (s = 0) or the destination (s = 1).  ws: bits[2][N][W].
__global__ void __launch_bounds__(LK_ST)
k_link_match(const float* __restrict__ boxes, const int* __restrict__ det_off, const int* __restrict__ frame_off,
             const float* __restrict__ tracks, const int* __restrict__ track_off, const long long* __restrict__ mat_off,
             float thr, int P, int F, int N, int NT, long long M, int max_dets, int max_tracks, int W,
             unsigned long long* __restrict__ bits, int* __restrict__ status)
{
    __shared__ float4 str[LK_MAXTR];
    Pair q;
    if (!pair_of(blockIdx.x, det_off, frame_off, track_off, mat_off, P, F, N, NT, M, max_dets, max_tracks, q)) {
        if (threadIdx.x == 0) *status = D2T_LINK_BAD_LAYOUT;
        return;
    }
    for (int i = threadIdx.x; i < q.ntr; i += LK_ST) str[i] = reinterpret_cast<const float4*>(tracks)[q.t0 + i];
    __syncthreads();
    const int nw = (q.ntr + 63) / 64;
    for (int i = threadIdx.x; i < q.Da + q.Db; i += LK_ST) {
        const int side = i < q.Da ? 0 : 1;
        const int n = side == 0 ? q.na + i : q.nb + (i - q.Da);
        const float4 box = reinterpret_cast<const float4*>(boxes)[n];
        unsigned long long* out = bits + ((size_t)side * N + n) * W;
        for (int w = 0; w < W; ++w) {
            unsigned long long m = 0;
            if (w < nw) {
                const int e = q.ntr - 64 * w < 64 ? q.ntr - 64 * w : 64;
                for (int j = 0; j < e; ++j)
                    if (iou_exceeds(box, str[64 * w + j], thr)) m |= 1ull << j;
            }
            out[w] = m;
        }
    }
}

// s[a][b] = (double)(float)(c_a + c_b) + psi: rows [LK_ROWS * blockIdx.y, +LK_ROWS) of pair blockIdx.x
__global__ void __launch_bounds__(LK_ST)
k_link_scores(const float* __restrict__ confs, const int* __restrict__ det_off, const int* __restrict__ frame_off,
              const int* __restrict__ track_off, const long long* __restrict__ mat_off,
              int P, int F, int N, int NT, long long M, int max_dets, int max_tracks, int W,
              const unsigned long long* __restrict__ bits, double* __restrict__ scores)
{
    Pair q;
    if (!pair_of(blockIdx.x, det_off, frame_off, track_off, mat_off, P, F, N, NT, M, max_dets, max_tracks, q)) return;   // (k_link_match reported it)
    const int r0 = LK_ROWS * blockIdx.y;
    if (r0 >= q.Da) return;
    const int rows = q.Da - r0 < LK_ROWS ? q.Da - r0 : LK_ROWS;
    const int nw = (q.ntr + 63) / 64;
    double* out = scores + q.m0;
    for (int e = threadIdx.x; e < rows * q.Db; e += LK_ST) {
        const int a = r0 + e / q.Db, b = e - (e / q.Db) * q.Db;
        const unsigned long long* ba = bits + (size_t)(q.na + a) * W;
        const unsigned long long* bb = bits + ((size_t)N + q.nb + b) * W;
        unsigned long long any = 0;
        for (int w = 0; w < nw; ++w) any |= ba[w] & bb[w];
        const float c = confs[q.na + a] + confs[q.nb + b];
        out[(size_t)a * q.Db + b] = (double)c + (any ? 1.0 : 0.0);
    }
}

// (value, index) order of the first maximum: a larger value wins; an equal one wins with a smaller index
__device__ __forceinline__ bool beats(double ov, int oi, double v, int i) { return ov > v || (ov == v && oi < i); }

__device__ __forceinline__ void wave_best(double& v, int& i)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double ov = __shfl_xor(v, s, 64);
        const int oi = __shfl_xor(i, s, 64);
        if (beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

struct LinkSmem {
    int off[LK_MAXF + 1];                     // node offsets of the problem's frames, relative to its first node
    double sv[LK_MAXD];                       // DP values of the source frame
    unsigned char slive[LK_MAXD];             // source not removed
    unsigned char stale[2][LK_MAXD];          // removed or changed value, by frame parity
    unsigned char dirty[LK_MAXD];
    short list[LK_MAXD];
    int cnt[LK_MAXD];                         // finite live entries in each column of the final frame's matrix
    double rv[LK_WAVES];
    int ri[LK_WAVES];
    int nlist, total, bad, winner, start, len, prev, done;
};

// One workgroup per problem: the whole extraction loop.  ws (by global node): val f64 | bp i32 (-1 = restart) | removed u8.
__global__ void __launch_bounds__(LK_T)
k_link_paths(const double* __restrict__ scores, const long long* __restrict__ mat_off, const double* __restrict__ init,
             const int* __restrict__ det_off, const int* __restrict__ frame_off, int P, int F, int N, long long M,
             int max_dets, int max_frames, int max_paths,
             int* __restrict__ out_start, int* __restrict__ out_len, double* __restrict__ out_score, int* __restrict__ out_nodes,
             int* __restrict__ out_count, int* __restrict__ out_status,
             double* __restrict__ val, int* __restrict__ bp, unsigned char* __restrict__ removed)
{
    __shared__ LinkSmem sm;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f0 = frame_off[p], T = frame_off[p + 1] - f0, g0 = f0 - p;
    // ---- the problem's layout, checked before anything is written
    bool bad = f0 < 0 || T < 1 || T > max_frames || f0 + T > F || g0 < 0 || g0 + T - 1 > F - P;
    if (tid == 0) sm.bad = 0;
    __syncthreads();
    if (!bad) {
        const int n0 = det_off[f0];
        for (int t = tid; t <= T; t += LK_T) {
            const int o = det_off[f0 + t];
            bad |= o < 0 || o > N || o < n0;
            if (t > 0) {
                const int d = o - det_off[f0 + t - 1];
                bad |= d < 0 || d > max_dets;
                if (!bad && t < T) {                                 // pair t-1 ends at frame t: its matrix
                    const int d2 = det_off[f0 + t + 1] - o;
                    const long long m0 = mat_off[g0 + t - 1];
                    bad |= d2 < 0 || d2 > max_dets || m0 < 0 || m0 + (long long)d * d2 > M;
                }
            }
            if (!bad) sm.off[t] = o - n0;
        }
    }
    if (bad) sm.bad = 1;                                             // (benign race: every writer stores 1)
    __syncthreads();
    if (sm.bad) {
        if (tid == 0) { out_count[p] = 0; out_status[p] = D2T_LINK_BAD_LAYOUT; }
        return;
    }
    const int n0 = det_off[f0], Np = sm.off[T];
    val += n0; bp += n0; removed += n0;
    auto D = [&](int t) { return sm.off[t + 1] - sm.off[t]; };
    auto mat = [&](int t) { return scores + mat_off[g0 + t - 1]; };  // the matrix into frame t >= 1
    for (int i = tid; i < Np; i += LK_T) {
        removed[i] = 0;
        bp[i] = -1;
        val[i] = i < sm.off[1] && init ? init[n0 + i] : 0.0;
    }
    __syncthreads();

    // Recompute frame t: every node when `all`, otherwise the removed ones and those whose best source is stale.
    auto step = [&](int t, bool all) {
        const int Da = D(t - 1), Db = D(t), sa = sm.off[t - 1], sb = sm.off[t];
        unsigned char* stp = sm.stale[(t - 1) & 1];
        unsigned char* stc = sm.stale[t & 1];
        for (int a = tid; a < Da; a += LK_T) { sm.sv[a] = val[sa + a]; sm.slive[a] = !removed[sa + a]; }
        if (tid == 0) sm.nlist = 0;
        __syncthreads();
        for (int b = tid; b < Db; b += LK_T) {
            bool d = all;
            stc[b] = 0;
            if (removed[sb + b]) {                                   // no live link reaches it: a restart at 0.0
                if (val[sb + b] != 0.0 || bp[sb + b] != -1) { val[sb + b] = 0.0; bp[sb + b] = -1; }
                stc[b] = 1;
                d = false;
            } else if (!d) {
                const int s = bp[sb + b];
                d = s >= 0 && stp[s];
            }
            sm.dirty[b] = d;
            if (d) sm.list[atomicAdd(&sm.nlist, 1)] = (short)b;
        }
        __syncthreads();
        const int nl = sm.nlist;
        const double* m = mat(t);
        __syncthreads();                                             // (everyone has read nlist before the next step resets it)
        if (nl == 0) return;
        if (4 * nl >= Db) {                                          // many: a thread per destination, rows read coalesced
            for (int b = tid; b < Db; b += LK_T) {
                if (!sm.dirty[b]) continue;
                double best = 0.0;
                int bi = -1;
                for (int a = 0; a < Da; ++a) {
                    const double s = sm.sv[a] + m[(size_t)a * Db + b];
                    if (sm.slive[a] && s > best) { best = s; bi = a; }
                }
                const double old = val[sb + b];
                val[sb + b] = best; bp[sb + b] = bi;
                stc[b] = __double_as_longlong(old) != __double_as_longlong(best);
            }
        } else {                                                     // few: a wave per destination, its lanes split the sources
            for (int j = wave; j < nl; j += LK_WAVES) {
                const int b = sm.list[j];
                double best = 0.0;
                int bi = -1;
                for (int a = lane; a < Da; a += 64) {
                    const double s = sm.sv[a] + m[(size_t)a * Db + b];
                    if (sm.slive[a] && s > best) { best = s; bi = a; }
                }
                wave_best(best, bi);
                if (lane == 0) {
                    const double old = val[sb + b];
                    val[sb + b] = best; bp[sb + b] = bi;
                    stc[b] = __double_as_longlong(old) != __double_as_longlong(best);
                }
            }
        }
        __syncthreads();
    };

    // The first maximum of frame t's values (all >= 0.0, never NaN) -> sm.winner
    auto pick = [&](int t) {
        const int Db = D(t), sb = sm.off[t];
        double best = -1.0;
        int bi = 0x7fffffff;
        for (int b = tid; b < Db; b += LK_T) {
            const double v = val[sb + b];
            if (v > best) { best = v; bi = b; }
        }
        wave_best(best, bi);
        if (lane == 0) { sm.rv[wave] = best; sm.ri[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            double v = sm.rv[0];
            int i = sm.ri[0];
            for (int w = 1; w < LK_WAVES; ++w)
                if (beats(sm.rv[w], sm.ri[w], v, i)) { v = sm.rv[w]; i = sm.ri[w]; }
            sm.winner = i;
        }
        __syncthreads();
    };

    int count = 0, used = 0, status = D2T_LINK_OK;
    // Write the path that ends at node w of frame t (thread 0); its nodes go to out_nodes reversed, then are flipped.
    auto emit = [&](int t, int w) {
        if (tid == 0) {
            int len = 0, node = w, u = t;
            while (node >= 0 && u >= 0 && len < Np - used) {         // (a path holds at most one node per frame)
                out_nodes[n0 + used + len] = node;
                ++len;
                node = bp[sm.off[u] + node];
                --u;
            }
            if (node >= 0) { sm.done = 1; sm.len = 0; }              // no room: cannot happen for a healthy extraction
            else {
                sm.len = len; sm.start = t - len + 1;
                sm.prev = len > 1 ? out_nodes[n0 + used + 1] : -1;
                out_start[n0 + count] = t - len + 1;
                out_len[n0 + count] = len;
                out_score[n0 + count] = val[sm.off[t] + w];
            }
        }
        __syncthreads();
        const int len = sm.len;
        int* nodes = out_nodes + n0 + used;
        for (int k = tid; k < len / 2; k += LK_T) {
            const int x = nodes[k];
            nodes[k] = nodes[len - 1 - k];
            nodes[len - 1 - k] = x;
        }
        __syncthreads();
    };

    if (tid == 0) sm.done = 0;
    for (int t = 1; t < T; ++t) step(t, true);                       // the full pass, once

    if (max_paths == 1) {                                            // viterbi(): the best path into the last frame
        if (D(T - 1) == 0) status = D2T_LINK_EMPTY;
        else {
            if (T == 1) {                                            // Python's max(): first element, replaced only by a greater one
                if (tid == 0) {
                    int i = 0;
                    for (int b = 1; b < D(0); ++b) if (val[b] > val[i]) i = b;
                    sm.winner = i;
                }
                __syncthreads();
            } else {
                pick(T - 1);
            }
            emit(T - 1, sm.winner);
            if (sm.len > 0) count = 1;
            else status = D2T_LINK_INTERNAL;
        }
    } else {
        for (int fin = T - 1; fin >= 1 && status == D2T_LINK_OK; --fin) {
            const int Da = D(fin - 1), Db = D(fin), sa = sm.off[fin - 1], sb = sm.off[fin];
            const double* m = mat(fin);
            if (tid == 0) sm.total = 0;
            for (int a = tid; a < Da; a += LK_T) sm.slive[a] = !removed[sa + a];
            __syncthreads();
            for (int b = tid; b < Db; b += LK_T) {
                int c = 0;
                if (!removed[sb + b])
                    for (int a = 0; a < Da; ++a) c += sm.slive[a] && __builtin_isfinite(m[(size_t)a * Db + b]);
                sm.cnt[b] = c;
                if (c) atomicAdd(&sm.total, c);
            }
            __syncthreads();
            while (sm.total > 0) {
                if (count >= Np) { status = D2T_LINK_INTERNAL; break; }  // every healthy extraction removes a live node
                pick(fin);
                const int w = sm.winner;
                if (removed[sb + w]) { status = D2T_LINK_NONTERMINATING; break; }   // the reference would repeat this forever
                emit(fin, w);
                if (sm.len == 0) { status = D2T_LINK_INTERNAL; break; }
                const int start = sm.start, len = sm.len, prev = sm.prev;
                for (int k = tid; k < len; k += LK_T) removed[sm.off[start + k] + out_nodes[n0 + used + k]] = 1;
                ++count;
                used += len;
                __syncthreads();
                if (tid == 0) sm.total -= sm.cnt[w];
                __syncthreads();
                if (tid == 0) sm.cnt[w] = 0;
                if (prev >= 0) {                                     // the row of the path's node in frame fin - 1 goes
                    for (int b = tid; b < Db; b += LK_T)
                        if (!removed[sb + b] && __builtin_isfinite(m[(size_t)prev * Db + b])) {
                            sm.cnt[b] -= 1;
                            atomicSub(&sm.total, 1);
                        }
                }
                // revisit frames max(start, 1)..fin: stale sources are the removed ones of the frame before
                const int t0 = start > 1 ? start : 1;
                for (int a = tid; a < D(t0 - 1); a += LK_T) sm.stale[(t0 - 1) & 1][a] = removed[sm.off[t0 - 1] + a];
                __syncthreads();
                for (int t = t0; t <= fin; ++t) step(t, false);
                __syncthreads();
            }
        }
        if (status == D2T_LINK_OK) {                                 // live frame-0 nodes with a finite init score, in order
            for (int c0 = 0; c0 < D(0); c0 += 64) {
                const int i = c0 + lane;
                const bool keep = i < D(0) && !removed[i] && __builtin_isfinite(val[i]);
                const unsigned long long bal = __ballot(keep);
                const int k = __popcll(bal & ((1ull << lane) - 1ull));
                if (wave == 0 && keep && count + k < Np && used + k < Np) {
                    out_start[n0 + count + k] = 0;
                    out_len[n0 + count + k] = 1;
                    out_score[n0 + count + k] = val[i];
                    out_nodes[n0 + used + k] = i;
                }
                count += __popcll(bal);
                used += __popcll(bal);
            }
        }
    }
    if (tid == 0) { out_count[p] = status == D2T_LINK_OK || status == D2T_LINK_NONTERMINATING ? count : 0; out_status[p] = status; }
}

}  // namespace

size_t link_scores_ws_bytes(int n_nodes, int max_tracks) { return al256((size_t)2 * n_nodes * words_of(max_tracks) * 8); }
size_t link_paths_ws_bytes(int n_nodes) { return al256((size_t)n_nodes * 8) + al256((size_t)n_nodes * 4) + al256((size_t)n_nodes); }

int link_scores_f32(const float* confs, const float* boxes, const int* det_off, const int* frame_off, const float* tracks,
                    const int* track_off, const long long* mat_off, float iou_thresh, int P, int F, int N, int n_tracks,
                    long long M, int max_dets, int max_tracks, double* scores, int* status, void* ws, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int), st);
    if (e != hipSuccess) return static_cast<int>(e);
    const int npairs = F - P;
    if (npairs == 0) return D2T_OK;
    const int W = words_of(max_tracks);
    auto* bits = static_cast<unsigned long long*>(ws);
    hipLaunchKernelGGL(k_link_match, dim3(npairs), dim3(LK_ST), 0, st, boxes, det_off, frame_off, tracks, track_off, mat_off,
                       iou_thresh, P, F, N, n_tracks, M, max_dets, max_tracks, W, bits, status);
    const int rb = max_dets > 0 ? (max_dets + LK_ROWS - 1) / LK_ROWS : 1;
    hipLaunchKernelGGL(k_link_scores, dim3(npairs, rb), dim3(LK_ST), 0, st, confs, det_off, frame_off, track_off, mat_off,
                       P, F, N, n_tracks, M, max_dets, max_tracks, W, bits, scores);
    e = hipGetLastError();
    return e == hipSuccess ? D2T_OK : static_cast<int>(e);
}

int link_paths_f64(const double* scores, const long long* mat_off, const double* init, const int* det_off, const int* frame_off,
                   int P, int F, int N, long long M, int max_dets, int max_frames, int max_paths,
                   int* out_start, int* out_len, double* out_score, int* out_nodes, int* out_count, int* out_status,
                   void* ws, hipStream_t st)
{
    char* w = static_cast<char*>(ws);
    double* val = reinterpret_cast<double*>(w); w += al256((size_t)N * 8);
    int* bp = reinterpret_cast<int*>(w); w += al256((size_t)N * 4);
    unsigned char* removed = reinterpret_cast<unsigned char*>(w);
    hipLaunchKernelGGL(k_link_paths, dim3(P), dim3(LK_T), 0, st, scores, mat_off, init, det_off, frame_off, P, F, N, M,
                       max_dets, max_frames, max_paths, out_start, out_len, out_score, out_nodes, out_count, out_status, val, bp, removed);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? D2T_OK : static_cast<int>(e);
}

}  // namespace d2t
