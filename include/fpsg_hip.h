/*
 * fpsg_hip.h -- C ABI of libfpsg_hip.so, the MI355X (gfx950) hot-path library.
 *
 * The reference (voidstrike/FPSG) has no native code of its own; its hot ops live in
 * third-party CUDA packages reached through Python imports.  Each entry point below
 * names the reference call site it replaces (paths relative to /root/reference).
 *
 * Conventions:
 *   - every pointer is a DEVICE pointer to a contiguous, 4-byte aligned buffer owned by
 *     the caller; the library never allocates, frees or keeps device memory;
 *   - a call only enqueues work on `stream` and returns (asynchronous);
 *   - return value 0 = success; >0 = hipError_t from the launch; <0 = argument check
 *     (FPSG_E_*); fpsg_last_error() gives a thread-local message for the last failure;
 *   - no C++ exception crosses the boundary; no global state besides that message (tuning variants
 *     are explicit arguments, never process-wide settings).
 *   - index outputs are int32 (the Python mirror widens to int64 where the reference
 *     API exposes int64).
 */
#ifndef FPSG_HIP_H
#define FPSG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* hipStream_t without dragging hip headers into C callers */
typedef void* fpsg_stream_t;

#define FPSG_ABI_VERSION 1

#define FPSG_E_NULL   (-1)  /* null pointer argument            */
#define FPSG_E_SHAPE  (-2)  /* non-positive / unsupported shape */
#define FPSG_E_ALIGN  (-3)  /* pointer not 4-byte aligned       */
#define FPSG_E_LIMIT  (-4)  /* size beyond a documented limit   */

int         fpsg_version(void);
const char* fpsg_last_error(void);
/* The byte size beyond which a pass takes its streaming (non-temporal) kernel form, as this build was compiled:
 * 300 MiB in libfpsg_hip.so, 0 in the tests' second build libfpsg_hip_stream.so (every pass streams).  A
 * compile-time constant; it tells a test which build it holds. */
size_t      fpsg_stream_threshold_bytes(void);

/* ---- K1: Chamfer sided distances ------------------------------------------------
 * Replaces kaolin.metrics.pointcloud.chamfer_distance (Kaolin 0.9.0, its CUDA
 * `sided_distance` forward), bound at src/models/few_shot.py:13,57 and called at
 * src/models/few_shot.py:110,117,167.
 *
 * xyz1 [B,N,3], xyz2 [B,M,3] fp32.  For every point of xyz1 the squared L2 distance to
 * its nearest point of xyz2 and that point's index (lowest index on ties), and vice
 * versa:  dist1,idx1 [B,N];  dist2,idx2 [B,M].
 * d(i,j) = fma(dz,dz, fma(dy,dy, dx*dx)),  dx = xyz2[j].x - xyz1[i].x  (fp32, RN).
 */
int fpsg_chamfer_fwd(const float* xyz1, const float* xyz2, int B, int N, int M,
                     float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                     fpsg_stream_t stream);

/* The same with an explicit kernel variant (micro-benchmarks, tests): (queries per lane, waves per
 * workgroup) 0=(1,16) 1=(2,16) 2=(4,8) 3=(8,4) 4=(4,4) 5=(2,8) 6=(2,4); -1 = automatic.  Results do
 * not depend on it. */
int fpsg_chamfer_fwd_variant(const float* xyz1, const float* xyz2, int B, int N, int M,
                             float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                             int cfg, fpsg_stream_t stream);

/* One-pass form of the same op (the default of the Python mirror for clouds of at most 4096 points):
 * every d(i,j) is evaluated once and serves both directions (d is bit-symmetric); 2-D tiles of
 * 64*R rows x W*cpw*16 candidates leave 32-bit partial keys in the caller's workspace (a tile's exact minimum with
 * its six lowest mantissa bits replaced by where inside the tile it was found), a second launch re-evaluates the
 * named range of every tile whose truncated minimum equals the smallest one and so recovers the exact distances and
 * first-minimum indices.  Bit-identical results to fpsg_chamfer_fwd.  Deterministic (no float atomics; the
 * workspace's contents before the call do not matter).
 * ws: fpsg_chamfer_workspace_bytes(B,N,M,variant) bytes, 8-byte aligned.  variant: -1 automatic,
 * else (R==8 ? 100 : 0) + 10*W + cpw with R in {4,8}, W in {1,2,4}, cpw in 1..9.  The workspace size
 * is 0 when this form does not apply: N or M > 4096, or (variant -1) fewer than ~7 pairs of
 * 2048-point clouds, where fpsg_chamfer_fwd's small workgroups fill the chip better.
 * fpsg_chamfer_fwd_tiled_losses: the same op plus K1l's three loss sums (fpsg_chamfer_losses below: same values, bit
 * for bit) -- the second launch also leaves every 256-point block's distance sum in the workspace, a one-workgroup
 * third launch adds them up; no separate pass over dist1 / dist2.  B <= 4096. */
size_t fpsg_chamfer_workspace_bytes(int B, int N, int M, int variant);
int fpsg_chamfer_fwd_tiled(const float* xyz1, const float* xyz2, int B, int N, int M,
                           float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                           void* ws, size_t ws_bytes, int variant, fpsg_stream_t stream);
int fpsg_chamfer_fwd_tiled_losses(const float* xyz1, const float* xyz2, int B, int N, int M,
                                  float* dist1, int32_t* idx1, float* dist2, int32_t* idx2,
                                  void* ws, size_t ws_bytes, int variant, int n_first, float w_first,
                                  float w_rest, float* out3, fpsg_stream_t stream);

/* Backward of the two sided distances w.r.t. both clouds (Kaolin's
 * sided_distance backward, reached through autograd from
 * src/trainNetwork.py:144 `ttl_loss.backward()`).
 * g1 [B,N], g2 [B,M] are the upstream gradients of dist1/dist2.
 * gxyz1 [B,N,3], gxyz2 [B,M,3] are fully overwritten.  Deterministic (Kaolin scatters with float
 * atomics, i.e. in no defined order).  Order fixed here, per output point i of cloud a:
 *   own term   ga_i = (2 g_a[i]) (a_i - b[idx_a[i]]);
 *   the sources j with idx_b[j] == i, in ascending j, are cut into blocks of 32; block k is summed
 *   from +0 by S_k = fma(2 g_b[j], a_i - b_j, S_k); then ga_i += S_0, += S_1, ... in block order.
 * fpsg_chamfer_bwd picks between the two kernels below (same results):
 *   _sorted: N, M <= 4096; one workgroup per (pair, side) inverts the argmin list by sorting
 *            (target, source) keys in LDS -- time independent of how many sources share a target;
 *   _scan  : any size; every 256-point tile scans the other side's argmin list. */
int fpsg_chamfer_bwd(const float* xyz1, const float* xyz2,
                     const int32_t* idx1, const int32_t* idx2,
                     const float* g1, const float* g2,
                     int B, int N, int M,
                     float* gxyz1, float* gxyz2, fpsg_stream_t stream);
int fpsg_chamfer_bwd_sorted(const float* xyz1, const float* xyz2,
                            const int32_t* idx1, const int32_t* idx2,
                            const float* g1, const float* g2,
                            int B, int N, int M,
                            float* gxyz1, float* gxyz2, fpsg_stream_t stream);
int fpsg_chamfer_bwd_scan(const float* xyz1, const float* xyz2,
                          const int32_t* idx1, const int32_t* idx2,
                          const float* g1, const float* g2,
                          int B, int N, int M,
                          float* gxyz1, float* gxyz2, fpsg_stream_t stream);

/* K1l: the episode's reconstruction losses from the distances of one fpsg_chamfer_fwd* call over B cloud pairs of which
 * the first n_first are the query pairs (src/models/few_shot.py:110-124: chamfer_distance(...).sum() per group, then
 * query_factor * q + support_factor * s).  out3 = { sum_{b < n_first} cd_b, sum_{b >= n_first} cd_b,
 * w_first * out3[0] + w_rest * out3[1] },  cd_b = mean_i dist1[b,i] + mean_j dist2[b,j].  B <= 4096.  Deterministic;
 * the summation order (also fpsg_chamfer_fwd_tiled_losses's and the oracle's oracle_chamfer_losses):
 *   a row (dist1[b,:] or dist2[b,:]) is cut into blocks of 256 consecutive values, values past the end count as +0;
 *   inside a block each of the four groups of 64 consecutive values is summed by the balanced binary tree over the
 *   position in the group (pairs at distance 1, then 2, 4, ... 32), block = ((T0 + T1) + T2) + T3;
 *   the row's sum adds its blocks in ascending order starting from +0;  cd_b = s1 * (1/N) + s2 * (1/M) with the
 *   reciprocals rounded to fp32 first (how PyTorch's GPU mean divides; equal to a division when N is a power of two);
 *   a group's sum (the pairs below n_first / the rest; a pair outside the group counts as +0): 64 partial sums
 *   p_l = cd_l + cd_(l+64) + ... in ascending order from +0, then the same balanced tree over l = 0..63;
 *   the total is w_first * q + w_rest * r, unfused. */
int fpsg_chamfer_losses(const float* dist1, const float* dist2, int B, int N, int M, int n_first,
                        float w_first, float w_rest, float* out3, fpsg_stream_t stream);
/* Its backward: g1 [B,N], g2 [B,M] (fully overwritten) = the gradients of the three values with respect to dist1 /
 * dist2 given the upstream gradients g_first, g_rest, g_total (device scalars; null = none), ready for fpsg_chamfer_bwd:
 *   g1[b,:] = g * (1/N), g2[b,:] = g * (1/M) (fp32 reciprocals, the bits of autograd's mean backward on the GPU),
 *   g = g_total * (b < n_first ? w_first : w_rest) + (b < n_first ? g_first : g_rest). */
int fpsg_chamfer_loss_grads(const float* g_first, const float* g_rest, const float* g_total, int B, int N, int M,
                            int n_first, float w_first, float w_rest, float* g1, float* g2, fpsg_stream_t stream);
/* fpsg_chamfer_loss_grads + fpsg_chamfer_bwd_sorted in one launch (N, M <= 4096): the per-pair constants are formed
 * inside the backward kernel, the two constant [B,N] / [B,M] arrays are never written or read.  Same bits. */
int fpsg_chamfer_bwd_losses(const float* xyz1, const float* xyz2, const int32_t* idx1, const int32_t* idx2,
                            const float* g_first, const float* g_rest, const float* g_total,
                            int B, int N, int M, int n_first, float w_first, float w_rest,
                            float* gxyz1, float* gxyz2, fpsg_stream_t stream);

/* ---- K3: kNN graph ----------------------------------------------------------------
 * Replaces `knn(x, k)` of src/dgcnn/model.py:13-20 (torch.matmul into a [B,N,N] matrix +
 * torch.topk).  x [B,C,N] fp32 channel-major (the reference's layout); idx [B,N,k] int32: for every point the k
 * points with the largest  pd_ij = (-|x_j|^2 + 2 x_i.x_j) - |x_i|^2, nearest first (self
 * included), equal values -> lower index first.  ws: caller scratch of fpsg_knn_workspace_floats(B,C,N) floats,
 * 16-byte aligned (squared norms + a zero-padded, point-major, k-interleaved copy of x whose 16-byte pieces are the
 * MFMA operands of four channel steps).
 * Two kernels, identical results (bit for bit the oracle's; deterministic, no atomics on global memory):
 *   - C <= 128 and k <= 24: the streaming kernel (knn_stream.hip) -- a workgroup owns 128 queries, the cloud's
 *     candidates pass once through LDS, a row keeps only the scores above a running lower bound of its k-th best;
 *   - otherwise (C <= 440, k <= 64): the score-tile kernel (knn.hip) -- 16 queries per workgroup, their scores
 *     against 2048 candidates at a time in LDS, longer clouds in chunks whose sorted top-k lists are merged.
 * fpsg_knn_ex: `layout` says how x is stored -- FPSG_KNN_CHANNEL_MAJOR [B,C,N] or FPSG_KNN_POINT_MAJOR [B,N,C]
 * (what the fused EdgeConv layers produce; only where the streaming kernel serves, FPSG_E_LIMIT otherwise);
 * `flags`: FPSG_KNN_FORCE_TILE selects the score-tile kernel, FPSG_KNN_FORCE_SLOW makes every wave of the streaming
 * kernel take its slow exact path (the one a row buffer that cannot be compacted falls back to) -- both for tests
 * and A/B timing.  fpsg_knn(x, ...) = fpsg_knn_ex(x, FPSG_KNN_CHANNEL_MAJOR, ..., 0).
 */
#define FPSG_KNN_CHANNEL_MAJOR 0
#define FPSG_KNN_POINT_MAJOR   1
#define FPSG_KNN_FORCE_TILE    1
#define FPSG_KNN_FORCE_SLOW    2
size_t fpsg_knn_workspace_floats(int B, int C, int N);
int fpsg_knn(const float* x, int B, int C, int N, int k, int32_t* idx, float* ws,
             fpsg_stream_t stream);
int fpsg_knn_ex(const float* x, int layout, int B, int C, int N, int k, int32_t* idx, float* ws,
                int flags, fpsg_stream_t stream);

/* ---- K4a: EdgeConv edge features (materialising form) ------------------------------
 * Replaces `get_graph_feature(x, k, idx)` of src/dgcnn/model.py:23-42.
 * out [B,2C,N,k]: out[b,c,n,j] = x[b,c,idx[b,n,j]] - x[b,c,n];  out[b,C+c,n,j] = x[b,c,n].
 */
int fpsg_edge_feature_fwd(const float* x, const int32_t* idx, int B, int C, int N, int k,
                          float* out, fpsg_stream_t stream);

/* Gradient of the above w.r.t. x (gx [B,C,N], fully overwritten).  The neighbour terms
 * are accumulated with fp32 atomics. */
int fpsg_edge_feature_bwd(const float* gout, const int32_t* idx, int B, int C, int N, int k,
                          float* gx, fpsg_stream_t stream);

/* ---- K2: EMD, approximate-assignment solver -------------------------------------
 * Stands where the reference calls neuralnet_pytorch.metrics.emd_loss through
 * emd_wrapper (src/models/utils.py:12-13, used at src/models/few_shot.py:168).
 * Auction-style soft assignment over 10 temperature levels (Fan/Su/Guibas approxmatch)
 * followed by the transport cost sum_kl match_kl * |xyz1_k - xyz2_l|; the N x M match
 * matrix is never stored.  cost [B].  gxyz1 [B,N,3] / gxyz2 [B,M,3] may each be NULL;
 * when given they receive d cost / d xyz with the assignment held constant (the
 * convention of the original matchcost gradient).  ws: caller scratch of
 * fpsg_emd_workspace_floats(B,N,M) floats, 16-byte aligned (per-point state and
 * coordinate-major copies of both clouds, rows padded to multiples of 4 points).
 * Deterministic (no float atomics).
 * fpsg_emd_approx_variant: `variant` -1 = automatic (what fpsg_emd_approx passes), else two bits that only act on
 * forward-only calls (both gradients NULL: the evaluation path): bit 0 = a level's assignment sweep and the next
 * level's row-normaliser sweep as ONE launch (same owners, same swept cloud; 21 sweeps per call instead of 30; the
 * assignment's exp(level d^2) is formed as the fourth power of the normaliser's exp(level/4 d^2)), bit 1 = four owner
 * points per wave instead of two.  Same values up to fp32 rounding of the exponentials (~4e-7 per weight).
 */
size_t fpsg_emd_workspace_floats(int B, int N, int M);
int fpsg_emd_approx(const float* xyz1, const float* xyz2, int B, int N, int M, float* cost,
                    float* gxyz1, float* gxyz2, float* ws, fpsg_stream_t stream);
int fpsg_emd_approx_variant(const float* xyz1, const float* xyz2, int B, int N, int M, float* cost,
                            float* gxyz1, float* gxyz2, float* ws, int variant, fpsg_stream_t stream);

/* ---- K12: exact EMD, forward auction with eps-scaling -------------------------------
 * The exact transport distance that K2 (approximate assignment) and K2b (Sinkhorn divergence) stand in
 * for: between equal-size clouds xyz1, xyz2 [B,N,3] fp32,  cost[b] = min over permutations a of
 * sum_i |xyz1_i - xyz2_a(i)|  (Euclidean, not squared, not divided by N), to within N * eps_final.
 * Evaluation metric only; the reference has no exact form (its emd_loss packages are absent).
 * One workgroup per pair; a Bertsekas forward auction (bidders = xyz1, objects = xyz2, prices start at 0)
 * over phases eps_0 = bbox diagonal / 4, eps_0 / 4, ... down to eps_final.  Outputs:
 *   cost [B]   sum_i |xyz1_i - xyz2_assign(i)| (fixed summation order);
 *   gap [B]    certificate cost - D, D = sum_i min_j (c_ij + p_j) - sum_j p_j the LP dual value of the final
 *              prices, so cost - gap <= exact EMD <= cost; 0 <= gap <= N * eps_final (up to fp32 rounding)
 *              when status = 0;
 *   assign [B,N] int32, a permutation of 0..N-1 (also when capped);
 *   status [B] int32: 0 = converged, 1 = the round cap max_rounds was hit (the assignment was completed
 *              with the free objects in index order; cost and gap still hold for it);
 *   gxyz1, gxyz2 [B,N,3] (each may be NULL): d cost / d xyz with the assignment held constant (K2's
 *              convention): (xyz1_i - xyz2_a(i)) / |xyz1_i - xyz2_a(i)|, 0 where that distance is 0, and its
 *              negative at a(i) for gxyz2;
 *   ws         fpsg_emd_exact_workspace_floats(B,N) device floats: per pair the int32 statistics (rounds in
 *              all, rounds of the last phase, phases, bits of eps_0).
 * Bounded work: at most max_rounds auction rounds per pair, no spin-wait, no communication between
 * workgroups.  Deterministic (bit-identical across runs).  1 <= N <= FPSG_EMD_EXACT_MAX_N; eps_final > 0
 * and finite; max_rounds >= 1; otherwise FPSG_E_SHAPE before any launch (FPSG_E_NULL for a null required
 * pointer).
 */
#define FPSG_EMD_EXACT_MAX_N 2048
size_t fpsg_emd_exact_workspace_floats(int B, int N);
int fpsg_emd_exact(const float* xyz1, const float* xyz2, int B, int N, float eps_final, int max_rounds,
                   float* cost, float* gap, int* assign, int* status,
                   float* gxyz1, float* gxyz2, float* ws, fpsg_stream_t stream);

/* ---- K13: all-pairs Chamfer matrix -----------------------------------------------------
 * Between every cloud of xyz1 [Na,N,3] and every cloud of xyz2 [Nb,M,3] (fp32, contiguous, device):
 *   out[a][b] = mean_i min_j d(xyz1[a,i], xyz2[b,j]) + mean_j min_i d(xyz2[b,j], xyz1[a,i]),
 *   d(p,q) = fma(dz,dz, fma(dy,dy, dx*dx)), dx = q.x - p.x, ...
 * i.e. chamfer_distance (K1, Kaolin 0.9.0's convention) of the pair.  Evaluation metric only (the set-level
 * generation metrics MMD / COV / 1-NNA); forward only, no indices, no per-point outputs, no workspace.
 * Output: out [Na,Nb] fp32.  xyz2 == NULL selects the symmetric mode, xyz1 against itself (Nb = Na and
 * M = N required): each unordered pair is evaluated once and mirrored; the diagonal is exactly 0.
 * Arithmetic: every per-point minimum is bit-identical to K1's dist1 / dist2.  Each of the two means is
 * S / n, S the sum of the n per-point minima of one cloud in a fixed order that depends on n alone:
 * 256 partial sums, partial t = the minima of points t*K .. t*K+K-1 added in ascending order (K = 2, 4, 8,
 * 16 for n <= 512, 1024, 2048, 4096), combined by a fixed tree.  That order is the only difference from
 * chamfer_distance.  out[a][b] = S_a / N + S_b / M.
 * Determinism: no floating-point atomics; out[a][b] is bitwise the same on every run and whatever Na, Nb,
 * slice or launch it was computed in; the matrix of (xyz2, xyz1) is bitwise the transpose of this one.
 * Errors, all before any launch: FPSG_E_NULL for a null xyz1 or out; FPSG_E_SHAPE for Na, Nb, N or M < 1
 * (or, in the symmetric mode, Nb != Na or M != N); FPSG_E_LIMIT for N or M > FPSG_CHAMFER_CROSS_MAX_N.
 */
#define FPSG_CHAMFER_CROSS_MAX_N 4096
int fpsg_chamfer_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, int M, float* out,
                       fpsg_stream_t stream);

/* ---- K14: all-pairs exact EMD matrix ---------------------------------------------------
 * Between every cloud of xyz1 [Na,N,3] and every cloud of xyz2 [Nb,N,3] (fp32, contiguous, device, equal N):
 * cost[a][b] = the exact EMD of the pair as fpsg_emd_exact computes it (sum of matched Euclidean distances,
 * not divided by N), by K12's auction (same bids, same eps schedule from the pair's own bounding box, same
 * caps): for the same eps_final and max_rounds, status and rounds equal K12's, and cost and gap are bitwise
 * K12's.  Evaluation metric only (MMD / COV / 1-NNA under EMD); forward only, no assignment, no gradients.
 * Outputs, all [Na,Nb]: cost, gap (cost - gap <= EMD <= cost), status (int32: 0 converged, 1 capped at
 * max_rounds and completed) and, when not NULL, rounds (int32: auction rounds of the pair in all).
 * xyz2 == NULL selects the symmetric mode, xyz1 against itself (Nb = Na): each unordered pair a < b is solved
 * once with xyz1[a] as bidders and mirrored; the diagonal is exact zeros (cost, gap, status, rounds 0).
 * ws: fpsg_emd_cross_workspace_bytes(Na,Nb,N) bytes, 8-byte aligned (the pair counter, zeroed on the
 * stream before the launch).  One workgroup per pair; persistent workgroups, no floating-point atomics:
 * every entry is bitwise the same whatever Na, Nb, slice or launch it was computed in.  Bounded work: at
 * most max_rounds rounds per pair, no spin-wait.
 * Errors, all before any launch: FPSG_E_NULL for a null xyz1, cost, gap, status or ws; FPSG_E_ALIGN for a
 * misaligned xyz2, rounds or ws; FPSG_E_SHAPE for Na, Nb or N < 1, Nb != Na in the symmetric mode, eps_final
 * not positive and finite, max_rounds < 1 or a workspace too small; FPSG_E_LIMIT for N > FPSG_EMD_EXACT_MAX_N.
 */
size_t fpsg_emd_cross_workspace_bytes(int Na, int Nb, int N);
int fpsg_emd_cross(const float* xyz1, const float* xyz2, int Na, int Nb, int N, float eps_final, int max_rounds,
                   float* cost, float* gap, int* status, int* rounds, void* ws, size_t ws_bytes,
                   fpsg_stream_t stream);

/* ---- K15: voxel-occupancy grid of a set of clouds (for the Jensen-Shannon divergence) ----------
 * The seventh column of the generation-metrics table (Achlioptas et al. 2018): the JSD between the occupancy
 * distributions of a generated and a reference set.  The published packages are not pinned; the definition
 * below is the specification.
 * xyz [S,N,3] fp32.  Grid of res^3 nodes (i,j,k) at -E + 2 E i / (res-1) per axis, E = half_extent, linear index
 * (i res + j) res + k.  in_sphere != 0: a node is retained iff (2i-(res-1))^2 + (2j-(res-1))^2 + (2k-(res-1))^2 <=
 * (res-1)^2 (integers); otherwise every node is retained.
 * Per point p, per axis, fp32 without fused multiply-add: t = fl(fl(p s) + c), s = fl((res-1) / (2E)),
 * c = fl((res-1) / 2) (formed in double, rounded once); n0 = clamp(rint(t), 0, res-1), round half to even.  The
 * point's cell is n0 if retained, else the retained node minimising d = fl(fl(fl(dx dx) + fl(dy dy)) + fl(dz dz)),
 * dx = fl(t_x - i), ..., ties to the lowest linear index.  A point with a NaN or infinite coordinate has no
 * cell (-1).
 * Outputs, all int32 and all ACCUMULATED INTO (the caller zeroes them once per set and may call again with more
 * clouds of the same set): counts [res^3] += points per cell; clouds_hit [res^3] += clouds of this call with at
 * least one point in the cell; outside [3] += {finite points with some |p| > E, finite points with
 * fl(fl(fl(x x) + fl(y y)) + fl(z z)) > fl(E E), non-finite points}.  cells [S,N] (may be NULL) = the cell of every
 * point, overwritten.  Integer atomics only: the results do not depend on launch order, slicing or accumulation.
 * No workspace: fpsg_occupancy_grid_workspace_bytes returns 0 and ws may be NULL.
 * Errors, all before any launch: FPSG_E_SHAPE for S or N < 1, res < 2, res = 2 with in_sphere, or a half_extent
 * that is not positive and finite (or so small that s overflows); FPSG_E_LIMIT for res >
 * FPSG_OCCUPANCY_MAX_RES; FPSG_E_NULL for a null xyz, counts, clouds_hit or outside; FPSG_E_ALIGN for a misaligned
 * pointer.
 */
#define FPSG_OCCUPANCY_MAX_RES 64
size_t fpsg_occupancy_grid_workspace_bytes(int S, int N, int res);
int fpsg_occupancy_grid(const float* xyz, int S, int N, int res, float half_extent, int in_sphere, int32_t* counts,
                        int32_t* clouds_hit, int32_t* outside, int32_t* cells, void* ws, size_t ws_bytes,
                        fpsg_stream_t stream);

/* ---- K16: farthest point sampling --------------------------------------------------------------
 * Picks n of a cloud's N points so that every next pick is the point farthest from those already picked.  The
 * definition below is the specification.
 * xyz [B,N,3] fp32; start [B] int32 or NULL (index 0 for every cloud); idx [B,n] int32; min_dist [B,n] fp32 or NULL.
 * Per cloud, with d(i,j) = fma(dz,dz, fma(dy,dy, dx dx)) on the fp32 coordinate differences (the squared distance
 * of K1 and K13, same bits):
 *   idx[0] = start[b];  min_dist[0] = +inf;  D_i = d(i, idx[0]) for every i;
 *   for t = 1 .. n-1:  idx[t] = the LOWEST i at which D_i is largest;  min_dist[t] = D_idx[t] (before the update);
 *                      D_i = min(D_i, d(i, idx[t])) for every i.
 * A picked point has D = 0 and is picked again only when every point has D = 0 (the cloud has fewer than n
 * distinct points): then the lowest index repeats.  That is defined behaviour, not an error.
 * Inputs are expected finite.  With a non-finite coordinate the indices are unspecified but in [0, N), and the
 * kernel ends after its n rounds like any other call: the loop count never depends on the data.  A start[b] outside
 * [0, N) is clamped into the range by the kernel (the host cannot see it).
 * Results are bitwise the same on every run, independent of B and of a cloud's position in the batch, and
 * idx[:, :m] of a call with n equals the call with m.  No atomics, no communication between workgroups.
 * No workspace: fpsg_fps_workspace_bytes returns 0 and ws may be NULL.
 * Errors, all before any launch: FPSG_E_SHAPE for B or N < 1 or n outside 1..N; FPSG_E_LIMIT for N >
 * FPSG_FPS_MAX_N; FPSG_E_NULL for a null xyz or idx; FPSG_E_ALIGN for a misaligned pointer.
 */
#define FPSG_FPS_MAX_N 16384
size_t fpsg_fps_workspace_bytes(int B, int N, int n);
int fpsg_fps(const float* xyz, int B, int N, int n, const int32_t* start, int32_t* idx, float* min_dist, void* ws,
             size_t ws_bytes, fpsg_stream_t stream);

/* ---- K17: distance profile of cloud pairs (F-score at distance thresholds, Hausdorff distance) ----
 * The item-level columns beside Chamfer (Tatarchenko et al., CVPR 2019): which share of one cloud lies within a
 * distance of the other.  The published scripts are not pinned; the definition below is the specification
 * (DESIGN.md K17).
 * dist1 [B,N], dist2 [B,M] fp32 squared distances -- K1's outputs, but any non-negative rows are valid; tau2 [T]
 * fp32 DEVICE array of squared thresholds, in any order.
 *   counts [B,2,T] int32, overwritten: counts[b][0][t] = #{i : dist1[b,i] <= tau2[t]}, counts[b][1][t] the same over
 *     dist2[b,:].  The compare is fp32 `<=`: a value equal to the threshold is counted, a NaN is counted nowhere.
 *   maxima [B,2] fp32, overwritten: max(0, max_i dist[b,i]) per direction, NaN entries ignored.  The square root is
 *     the caller's (in double, on the host side), so the output is exact.
 * Exact (integers, and a maximum has no order); pair b's outputs are bitwise the same on every run, whatever B is
 * and wherever the pair sits in the batch.  No atomics, no workspace, no communication between workgroups; every
 * loop count depends on N, M and T only.  The call only enqueues work on `stream` (it can be captured in a graph).
 * Errors, all before any launch: FPSG_E_SHAPE for B, N, M or T < 1; FPSG_E_LIMIT for T > FPSG_PROFILE_MAX_T;
 * FPSG_E_NULL for any null pointer; FPSG_E_ALIGN for a misaligned pointer.
 */
#define FPSG_PROFILE_MAX_T 16
int fpsg_dist_profile(const float* dist1, const float* dist2, int B, int N, int M, const float* tau2, int T,
                      int32_t* counts, float* maxima, fpsg_stream_t stream);

/* ---- K18: density-aware Chamfer distance of cloud pairs -------------------------------------------
 * DCD (Wu et al., NeurIPS 2021, "Density-aware Chamfer Distance as a Comprehensive Metric for Point Cloud
 * Completion"): Chamfer's nearest-neighbour terms, bounded to [0, 1] by an exponential and divided by the number of
 * queries that chose the same nearest neighbour.  The published package is not pinned; the definition below is the
 * specification (parity UNPINNED).
 * Inputs are K1's outputs for B pairs of clouds p1 [N,3], p2 [M,3]: dist1, idx1 [B,N] (squared distance to, and index
 * in p2 of, the nearest point, lowest index on ties), dist2, idx2 [B,M] the same the other way.  Per pair:
 *   deg2[j] = #{ i : idx1[i] == j }        int32 [M]   (how many points of p1 chose p2[j])
 *   deg1[i] = #{ j : idx2[j] == i }        int32 [N]
 *   q1[i]   = exp(-alpha * d1[i]) / float(deg2[idx1[i]])          (deg >= 1 there by construction)
 *   q2[j]   = exp(-alpha * d2[j]) / float(deg1[idx2[j]])
 *   side1   = (sum_i (1 - q1[i])) * (1/N)      side2 = (sum_j (1 - q2[j])) * (1/M)
 *   dcd     = 0.5 * (side1 + side2)
 *   w1[i]   = d dcd / d d1[i] = (alpha * q1[i]) * (0.5 * (1/N))    w2[j] likewise with 1/M   (counts held constant)
 * alpha multiplies the SQUARED distance.  fp32 throughout: exp(-x) is the hardware base-2 exponential of
 * -((alpha * d) * log2(e)), each product rounded (a result below 2^-126 is +0); the division is IEEE; 1/N and 1/M are
 * rounded to fp32 first (as K1l).  The row sums use K1l's order: a row of terms is cut into blocks of 256 consecutive
 * values (past the end: +0), inside a block each of the four groups of 64 is summed by the balanced binary tree over
 * the position in the group, block = ((T0 + T1) + T2) + T3, and the blocks are added in ascending order from +0.
 * Outputs, all overwritten: out [B]; sides [B,2] = (side1, side2); deg1 [B,N], deg2 [B,M] int32; w1 [B,N], w2 [B,M]
 * fp32, each may be NULL (not wanted).
 * Special values: an index outside [0, M) (idx1) or [0, N) (idx2) is counted nowhere, reads and writes no memory
 * and gives q = 0 (term 1, weight 0) whatever its distance; a NaN distance with a valid index gives a NaN term and so
 * a NaN side and dcd for its pair only.  The entry point is memory-safe on any int32 index input.
 * Integer counts are exact; the float results are bitwise the same on every run, whatever B is and wherever the pair
 * sits in the batch; the two sides go through one routine, so swapping (dist1, idx1, N) with (dist2, idx2, M) swaps
 * sides, deg and w and leaves out bitwise unchanged.  One launch, one workgroup per pair, integer LDS atomics only,
 * no workspace, no communication between workgroups.  The call only enqueues work on `stream` (no host read; it
 * can be captured in a graph).
 * Errors, all before any launch: FPSG_E_NULL for a null pointer other than w1 / w2; FPSG_E_SHAPE for B, N or M < 1;
 * FPSG_E_LIMIT for N or M > FPSG_DCD_MAX_N (the in-degree histogram of one cloud lives in 64 KB of LDS); FPSG_E_ALIGN
 * for a misaligned pointer.
 */
#define FPSG_DCD_MAX_N 16384
int fpsg_dcd(const float* dist1, const int32_t* idx1, const float* dist2, const int32_t* idx2, int B, int N, int M,
             float alpha, float* out, float* sides, int32_t* deg1, int32_t* deg2, float* w1, float* w2,
             fpsg_stream_t stream);

/* ---- K21: repulsion regulariser of a cloud against itself --------------------------------------------
 * PU-Net's repulsion term (Yu et al., CVPR 2018): every point is charged for its k nearest neighbours in its OWN
 * cloud, eta(r) w(r) = -r exp(-r^2 / h^2).  The published code is not pinned; the definition below is the specification
 * (parity UNPINNED).  Inputs: B clouds xyz [N,3] fp32, 1 <= k <= FPSG_REPULSION_MAX_K, k <= N - 1, h > 0.
 *   d2(i,j)  = fma(dz,dz, fma(dy,dy, dx*dx)), dx = x_j - x_i (K1's sq_dist: bitwise symmetric in i and j)
 *   K(i)     = the k indices j != i with the smallest (d2(i,j), j) in lexicographic order (ties: the lower index),
 *              stored nearest first: nbr_idx [B,N,k] int32, nbr_d2 [B,N,k] fp32.  j == i is skipped by index, so a
 *              duplicate of point i is a neighbour of i at distance 0
 *   r        = sqrt(d2) where d2 > 1e-12, else 1e-6          (= sqrt(max(d2, 1e-12)))
 *   rho(d2)  = -(r * exp(-d2 / h^2))
 *   rho'(d2) = -(e / (2 r) - (e r) / h^2), e = exp(-d2 / h^2), where d2 > 1e-12; 0 elsewhere (duplicates push nobody)
 *   value[b] = (1 / (N k)) sum_i sum_{j in K(i)} rho(d2(i,j))                  in [-h / sqrt(2 e), 0]
 *   gxyz[j]  = gvalue[b] (2 / (N k)) [ sum_{m in K(j)} rho'(d2(j,m)) (x_j - x_m)
 *                                      + sum_{i : j in K(i)} rho'(d2(i,j)) (x_j - x_i) ]
 * (the lists are piecewise constant: no gradient flows through the selection).  fp32 throughout: 1 / h^2 is formed
 * in double on the host, rounded to fp32 and kept finite; exp(-x) is the hardware base-2 exponential of
 * -((d2 * (1/h^2)) * log2(e)) (a result below 2^-126 is +0); sqrt and 1 / r are the hardware instructions.
 * Orders: a point's k terms of the value are added as a balanced tree over eight slots (absent: +0); 64 consecutive
 * points by the balanced tree over the position; 256 consecutive points as (w0 + w1) + (w2 + w3); these partials in
 * ascending order from +0; the product with 1 / (N k) (rounded to fp32) last.  A point's gradient starts from +0,
 * takes its own k terms in list order, then the reverse terms in ascending i, each as fma(rho', x_j - x_other, acc);
 * the product with gvalue[b] * (2 / (N k)) last.  gxyz is written, not accumulated.
 * The backward takes the lists as written by the forward: j is in K(i) exactly where (d2(i,j), j) <=
 * (nbr_d2[i,k-1], nbr_idx[i,k-1]) lexicographically and i != j, with d2 recomputed; a row whose k-th index is outside
 * [0, N) holds nobody, and an own index outside [0, N) is skipped: no index is dereferenced unchecked.  Coordinates
 * that are not finite give unspecified values for their cloud, never an access out of bounds.
 * Bitwise the same on every run, whatever B is and wherever the cloud sits in the batch; no atomics.  The forward is
 * two launches (the sweep; one thread per cloud adds the partials), the backward one; the workspace holds the
 * forward's partials.  The calls only enqueue work on `stream` (no host read; they can be captured in a graph).
 * Errors, all before any launch, shape and limit checks in front of the pointer checks: FPSG_E_SHAPE for B < 1, k
 * outside 1..8, N < k + 1, h not positive and finite, or a workspace smaller than fpsg_repulsion_workspace_bytes;
 * FPSG_E_LIMIT for N > FPSG_REPULSION_MAX_N; FPSG_E_NULL for a null pointer; FPSG_E_ALIGN for a misaligned one.
 * fpsg_repulsion_workspace_bytes returns 0 for a shape the entries refuse.
 */
#define FPSG_REPULSION_MAX_N 16384
#define FPSG_REPULSION_MAX_K 8
size_t fpsg_repulsion_workspace_bytes(int B, int N, int k);
int fpsg_repulsion_fwd(const float* xyz, int B, int N, int k, float h, int32_t* nbr_idx, float* nbr_d2, float* value,
                       void* workspace, size_t workspace_bytes, fpsg_stream_t stream);
int fpsg_repulsion_bwd(const float* xyz, const int32_t* nbr_idx, const float* nbr_d2, const float* gvalue, int B, int N,
                       int k, float h, float* gxyz, fpsg_stream_t stream);

/* ---- K22: sliced Wasserstein distance with its gradient and matchings ----------------------------------
 * The squared 2-Wasserstein distance of the clouds' projections on L given directions, averaged (Bonneel et al. 2015;
 * the cheap transport loss of the point-cloud literature).  Inputs: B pairs xyz1, xyz2 [N,3] fp32 with the SAME N,
 * directions dirs [L,3] fp32 shared by every pair, used as given (not normalised).  DESIGN.md K22.
 *   key      k = fl(fl(fl(x tx) + fl(y ty)) + fl(z tz)) + 0.0f      (fp32, this order; the last addition turns -0 into +0)
 *   pi1, pi2 per pair and direction: the N points of cloud 1 (2) ascending by (key, index), ties to the lower index;
 *            perm1 / perm2 [B,L,N] int32 hold pi1[r] / pi2[r] at rank r
 *   d_r      = k1[pi1[r]] - k2[pi2[r]]
 *   value[b] = 1 / (L N) sum_l sum_r d_r^2
 *   gxyz1[b, pi1[r]] += 2 / (L N) d_r theta_l          gxyz2[b, pi2[r]] -= 2 / (L N) d_r theta_l
 * gxyz1 / gxyz2 [B,N,3] are the gradient of value[b] with the matchings held constant (they are piecewise constant);
 * they are written, not accumulated, and either may be NULL, as may perm1 / perm2: the other outputs keep their bits.
 * The orders are total, so every output is determined: bitwise the same on every run, whatever B is and wherever the
 * pair sits in the batch, and value[b] is bitwise unchanged when the points of either cloud are permuted.  Orders of
 * the sums: the L directions are split over G = min(ceil(L / 8), 16) workgroups per pair, group g taking directions
 * [g L / G, (g + 1) L / G).  Inside a group the thread of rank r (and r + T, T = max(64, P / 2) threads, P the power
 * of two >= max(N, 64)) adds its d_r^2 in ascending direction, the 64 threads of a wave are added by the balanced tree
 * over the lane, the waves in ascending order; a gradient row takes its terms d_r theta (one product, one addition
 * each, from +0) in ascending direction.  The G partials are added in ascending g from +0 and multiplied by
 * 1 / (L N) resp. 2 / (L N), formed in double and rounded to fp32.  No atomics.
 * The sort is a bitonic network over P slots in LDS on 64-bit words (monotone image of the key << 32 | index); slots
 * N .. P - 1 hold sentinels above every real word, a NaN's included, which never reach d_r, the matchings or the
 * gradients.  Its control flow does not depend on the data: a coordinate or direction that is not finite gives
 * non-finite or unspecified values for the pairs it touches (a NaN key sorts behind +inf, or in front of -inf with the
 * sign bit set), never an access out of bounds, and leaves every other pair's bits alone.
 * Two launches (the groups; the sum of their partials).  The call only enqueues work on `stream` (no host read; it can
 * be captured in a graph).  ws: fpsg_swd_workspace_bytes(B, N, L) bytes, 4-byte aligned, contents unspecified.
 * Errors, all before any launch: FPSG_E_SHAPE for B, N or L < 1 or a workspace that is too small; FPSG_E_LIMIT for
 * N > FPSG_SWD_MAX_N, L > FPSG_SWD_MAX_L or B > FPSG_SWD_MAX_B; FPSG_E_NULL for a null xyz1, xyz2, dirs, value or ws;
 * FPSG_E_ALIGN for a misaligned pointer.  fpsg_swd_workspace_bytes returns 0 for a shape the entry refuses.
 */
#define FPSG_SWD_MAX_N 2048
#define FPSG_SWD_MAX_L 1024
#define FPSG_SWD_MAX_B 65535
size_t fpsg_swd_workspace_bytes(int B, int N, int L);
int fpsg_swd(const float* xyz1, const float* xyz2, const float* dirs, int B, int N, int L, float* value, float* gxyz1,
             float* gxyz2, int32_t* perm1, int32_t* perm2, void* ws, size_t ws_bytes, fpsg_stream_t stream);

/* ---- K24: expansion penalty of a multi-patch cloud (per-patch minimum spanning trees) -----------------
 * MSN's expansion penalty (Liu et al., AAAI 2020): the cloud is K patches of P consecutive points; each patch is
 * charged for the edges of its minimum spanning tree that are much longer than the tree's mean edge.  The published
 * code is not pinned; the definition below is the specification (parity UNPINNED).  Inputs: B clouds
 * xyz [N,3] fp32, 2 <= P <= FPSG_EXPANSION_MAX_P, N % P == 0, K = N / P, patch q = rows q P .. q P + P - 1, lambda >= 1.
 *   d2(u,v)  = K1's sq_dist: fma(dz,dz, fma(dy,dy, dx*dx)), dx = x_v - x_u (bitwise symmetric, never negative)
 *   T_q      = Prim's tree from local vertex 0 under d2: every non-tree vertex keeps a key (the smallest d2 to a tree
 *              vertex) and a parent; a later-added tree vertex replaces them only where its d2 is STRICTLY smaller (on
 *              ties the earlier-added vertex stays the parent); each step adds the non-tree vertex with the smallest
 *              (key, local index) in lexicographic order
 *   parent [B,N] int32: local index, -1 at each patch's vertex 0;  edge_d2 [B,N] fp32: the final key, 0 at vertex 0;
 *   order [B,N] int32: the step at which the vertex was added, 0 at vertex 0
 *   r_v      = sqrt(edge_d2[v])                                   (correctly rounded)
 *   l_q      = (sum_v r_v) / (P - 1)                              -> mean_len [B,K]
 *   v is penalised iff r_v > lambda * l_q (strictly; one fp32 product): with every point identical, with P = 2 or
 *              with all edges equal nothing is penalised
 *   E_q      = (sum_{v penalised} r_v) / (P - 1)
 *   value[b] = (sum_q E_q) / K                                    in [0, inf)
 *   gxyz[u]  = gvalue[b] (1 / (K (P - 1))) [ [u penalised] (x_u - x_par(u)) / r_u
 *                                            + sum_{v : par(v) = u, v penalised} (x_u - x_v) / r_v ]
 * (the tree, the penalised set and l_q are held constant: no gradient flows through them).  A penalised edge has r > 0,
 * so no floor is needed and duplicates give no NaN.  fp32 throughout; the divisions are fp32 divisions.
 * Orders: vertex v = t + 64 s belongs to lane t, slot s.  A sum over a patch's vertices adds each lane's slots in
 * ascending s from +0, then the 64 lanes by the balanced tree over the lane; the division by P - 1 follows.  A cloud's
 * K values E_q are added in ascending q from +0, the division by K last.  A gradient row starts from +0, takes its own
 * edge's term, then the child terms in ascending v, each term formed as a difference and a division per axis and
 * added; the product with gvalue[b] * (1 / (K (P - 1))) (formed in double, rounded to fp32) last.  gxyz is written,
 * not accumulated.
 * The backward recomputes sqrt(edge_d2[v]) > lambda * mean_len[b,q] -- the forward's expression on the forward's bits --
 * and skips every v whose parent is outside [0, P) or whose length is not positive: it is safe on any int32 / fp32
 * arrays.  With coordinates that are not finite the patch's results are unspecified, but the loop still ends after
 * P - 1 steps and every stored index is inside [0, P) (or the root's -1); no access goes out of bounds.
 * Bitwise the same on every run, whatever B is and wherever the cloud sits in the batch or the patch in the cloud; no
 * atomics.  One wavefront owns one patch.  The forward is two launches (the trees; one thread per cloud adds the
 * partials), the backward one; the workspace holds the forward's B K partials.  The calls only enqueue work on
 * `stream` (no host read; they can be captured in a graph).
 * Errors, all before any launch, shape and limit checks in front of the pointer checks: FPSG_E_SHAPE for B < 1, P < 2,
 * N not a positive multiple of P, lambda not finite or < 1, or a workspace smaller than
 * fpsg_expansion_workspace_bytes; FPSG_E_LIMIT for P > FPSG_EXPANSION_MAX_P or N > FPSG_EXPANSION_MAX_N; FPSG_E_NULL
 * for a null pointer; FPSG_E_ALIGN for a misaligned one.  fpsg_expansion_workspace_bytes returns 0 for a shape the
 * entries refuse.
 */
#define FPSG_EXPANSION_MAX_P 1024
#define FPSG_EXPANSION_MAX_N 16384
size_t fpsg_expansion_workspace_bytes(int B, int N, int P);
int fpsg_expansion_fwd(const float* xyz, int B, int N, int P, float lambda, int32_t* parent, float* edge_d2,
                       int32_t* order, float* mean_len, float* value, void* workspace, size_t workspace_bytes,
                       fpsg_stream_t stream);
int fpsg_expansion_bwd(const float* xyz, const int32_t* parent, const float* edge_d2, const float* mean_len,
                       const float* gvalue, int B, int N, int P, float lambda, float* gxyz, fpsg_stream_t stream);

/* ---- K25: uniform loss of a cloud (ball query, nearest neighbour inside a ball) -------------------------
 * PU-GAN's uniform loss (Li et al., ICCV 2019, sec. 3.3): balls of several sizes around seed points; each ball is
 * charged by how far its point count is from the expected count (imbalance) times how far its members' nearest-
 * neighbour distances are from the expected spacing (clutter).  The published code is not pinned; the definition below
 * is the specification (parity UNPINNED).  Inputs: B clouds xyz [N,3] fp32; seeds [B,S] int32 indices
 * into the own cloud; percent [T] fp32, a HOST array read during the call, each p_t in (0, 1], T <= FPSG_UNIFORM_MAX_T;
 * a scale radius R > 0; a cap C on the retained members of a ball, 64, 128 or 256.
 *   r2_t     = fp32(p_t R R), area_t = fp32((2 pi / sqrt 3) r2_t), nhat_t = fp32(N p_t): each product formed in double
 *              on the host and rounded once (nhat assumes a surface of area pi R^2, as PU-GAN does)
 *   d2(i,j)  = K1's sq_dist: fma(dz,dz, fma(dy,dy, dx*dx)) (bitwise symmetric, never negative)
 *   ball(j,t)= the ascending-index list of all i with d2(i, seeds[j]) <= r2_t (fp32 <=: a point exactly on the sphere
 *              is inside, the seed is its own member, a NaN distance is outside); c = the full count -> count [B,T,S]
 *              int32; the first m = min(c, C) members are retained -> member [B,T,S,C] int32, -1 behind them
 *   e_i      = for a retained member i the minimum of d2(i, i') over the OTHER retained members i', nn_i the lowest
 *              such index -> nn_d2, nn [B,T,S,C] at i's slot; +inf and -1 behind the list and where m = 1
 *   d_i      = sqrt(e_i) (correctly rounded);  dhat = sqrt(area_t / float(c)): the hexagonal-packing spacing of c
 *              points in the ball's disc
 *   term_i   = (d_i - dhat)^2 / dhat, and exactly dhat where e_i == 0 (a duplicate; it has no gradient)
 *   U(j,t)   = ((float(c) - nhat_t)^2 / nhat_t) * sum_i term_i over the retained members -> ball_value [B,T,S];
 *              0 where m < 2 and where seeds[j] is outside [0, N): such a seed owns an empty ball (c = 0, nothing read)
 *   per_percent[b,t] = (sum_j U(j,t)) / S;    value[b] = (sum_t sum_j U(j,t)) / (T S)
 *   gxyz[i]  = gvalue[b] (1 / (T S)) sum over the balls that retain i of
 *                [e_i > 0] s_i (x_i - x_nn_i)  +  sum_{i' retained, nn_i' = i, e_i' > 0} s_i' (x_i - x_i'),
 *              s_i = ((2 w / dhat) (d_i - dhat)) / d_i, w = (float(c) - nhat_t)^2 / nhat_t
 * (counts, lists and nn choices are piecewise constant: gradient flows through the d_i only).  fp32 throughout; the
 * divisions and square roots are IEEE.
 * Orders: retained member q (its place in the list) belongs to lane q % 64, slot q / 64 of its wavefront.  A ball's sum
 * adds each lane's slots in ascending order from +0, then the 64 lanes by the balanced tree over the lane; the product
 * with w follows.  A row (b, t) adds U(j, t), j = l, l + 64, ... in ascending order from +0 per lane l, then the lanes by
 * the same tree; the division by S gives per_percent.  A cloud's T row sums are added in ascending t from +0 and
 * divided by float(T) * float(S).  A gradient row starts from +0 and walks the balls in ascending (t, j); in a ball that
 * retains the point it takes its own term, then the terms of the members whose nn it is in list order, each as
 * fma(s, x_i - x_other, acc) per axis; the product with gvalue[b] * (1 / (T S)) (formed in double, rounded to fp32)
 * last.  gxyz is written, not accumulated.
 * The backward repeats the forward's compare d2(i, seeds[j]) <= r2_t on the same bits and finds the point's slot in
 * the ascending list; it takes count, member, nn and nn_d2 as the forward wrote them but is safe on any int32 / fp32
 * contents: a count is clamped to the cap, a ball with fewer than two retained members or a seed outside [0, N) is
 * skipped, as is every member or nn index outside [0, N) and every nn_d2 that is not positive.  Coordinates that are
 * not finite give unspecified values for their own cloud only, never an access out of bounds.
 * Bitwise the same on every run, whatever B is and wherever the cloud sits in the batch; no atomics.  Every loop
 * count depends on N, S, T and C only.  One wavefront owns one (cloud, seed).  The forward is three launches (the
 * balls; one wave per (cloud, percentage) adds a row; one thread per cloud adds the rows), the backward one (one thread
 * per point); the workspace holds the forward's B T row sums.  The calls only enqueue work on `stream` (no host
 * read; they can be captured in a graph).
 * Errors, all before any launch, in this order: FPSG_E_SHAPE for B, S or T < 1, N < 2, S > N, a radius not positive and
 * finite, a cap other than 64, 128 or 256; FPSG_E_LIMIT for N > FPSG_UNIFORM_MAX_N or T > FPSG_UNIFORM_MAX_T;
 * FPSG_E_NULL for a null percent (it is read next); FPSG_E_SHAPE for a percentage outside (0, 1] or not finite;
 * FPSG_E_NULL for any other null pointer, FPSG_E_ALIGN for a misaligned one; FPSG_E_SHAPE for a workspace smaller than
 * fpsg_uniform_workspace_bytes, which returns 0 for a shape the entries refuse.
 */
#define FPSG_UNIFORM_MAX_N 16384
#define FPSG_UNIFORM_MAX_T 8
#define FPSG_UNIFORM_MAX_MEMBERS 256
size_t fpsg_uniform_workspace_bytes(int B, int N, int S, int T, int cap);
int fpsg_uniform_fwd(const float* xyz, const int32_t* seeds, int B, int N, int S, const float* percent, int T,
                     float radius, int cap, int32_t* count, int32_t* member, int32_t* nn, float* nn_d2,
                     float* ball_value, float* per_percent, float* value, void* workspace, size_t workspace_bytes,
                     fpsg_stream_t stream);
int fpsg_uniform_bwd(const float* xyz, const int32_t* seeds, const int32_t* count, const int32_t* member,
                     const int32_t* nn, const float* nn_d2, const float* gvalue, int B, int N, int S, int T,
                     const float* percent, float radius, int cap, float* gxyz, fpsg_stream_t stream);

/* ---- K4b: fused EdgeConv (gather + BatchNorm statistics + max over k) -----------------
 * Replaces the chain get_graph_feature -> Conv2d 1x1 -> BatchNorm2d -> LeakyReLU -> max_k of
 * src/dgcnn/model.py:23-42,53-56,63-76 without materialising [B,2C,N,k].  The caller first
 * forms PQ [B,N,2*Co] = x^T [W1 ; W2-W1]^T (one GEMM): y(n,j) = P[idx[n,j]] + Q[n].
 *   fwd : sgn [Co]: >= 0 take max_j, < 0 take min_j per channel (only the sign is used: pass BN's gamma);
 *         ysel [B,N,Co] selected extreme of y over j; jsel [B,N,Co] uint8 its slot j (first on
 *         ties); s1 [B,N,Co] = sum_j y (NULL to skip); part [fpsg_edgeconv_blocks(B,N,Co)][2][Co]
 *         per-workgroup sums of y and y^2 for the BatchNorm statistics (NULL to skip).
 *   bwd : dzs [B,N,Co] = dL/dz * scale at the selected edge; rev [B,N*k] edge ids n*k+j sorted
 *         by destination idx (ascending id inside a destination), off [B,N+1] offsets into rev;
 *         coef [3][Co] = (A, Bc, mu) BatchNorm statistic terms (s1 == NULL: eval mode, coef
 *         ignored).  dPQ [B,N,2*Co] is fully overwritten.  Deterministic (no float atomics).
 * Co must be 64, 128 or 256; float buffers 16-byte aligned.
 */
int fpsg_edgeconv_blocks(int B, int N, int Co);
int fpsg_edgeconv_fwd(const float* PQ, const int32_t* idx, const float* sgn, int B, int N, int k,
                      int Co, float* ysel, uint8_t* jsel, float* s1, float* part,
                      fpsg_stream_t stream);
int fpsg_edgeconv_bwd(const float* dzs, const uint8_t* jsel, const float* PQ, const float* s1,
                      const int32_t* rev, const int32_t* off, const float* coef, int B, int N, int k,
                      int Co, float* dPQ, fpsg_stream_t stream);

/* The in-edge lists fpsg_edgeconv_bwd gathers through, from the neighbour lists idx [B][N][k] (values in [0,N)):
 * rev [B][N*k] = the edges e = n*k + j grouped by destination idx[n][j], ascending e inside a group (the backward's
 * summation order); off [B][N+1] = first slot of every destination's group, off[N] = N*k.  Replaces what autograd's
 * index backward of get_graph_feature's gather (src/dgcnn/model.py:30-56) does with atomics.  One workgroup per cloud,
 * a stable counting sort in LDS; deterministic.  Limits: N*k <= 65535 and N small enough for the LDS --
 * fpsg_edgeconv_reverse_graph_fits(N,k) answers 1 when both hold (the Python mirror sorts with torch otherwise).
 * Entries of idx outside [0,N) are skipped (their slots of rev stay unwritten). */
int fpsg_edgeconv_reverse_graph_fits(int N, int k);
int fpsg_edgeconv_reverse_graph(const int32_t* idx, int B, int N, int k, int32_t* rev, int32_t* off,
                                fpsg_stream_t stream);
/* The elementwise halves around them, on point-major [rows = B*N, Co] tensors: fpsg_edgeconv_act = the BatchNorm
 * affine form + LeakyReLU of the selected neighbour sum, out = lrelu(fma(ysel, scale[c], shift[c])) (one pass instead
 * of addcmul + leaky_relu); fpsg_edgeconv_bwd_prep = the head of the backward: z re-derived with the same arithmetic,
 * dz = g * lrelu'(z), dzs = dz * scale[c] for fpsg_edgeconv_bwd, and part [fpsg_edgeconv_prep_blocks(rows)][2][Co] =
 * per-workgroup sums of dz and dz * ysel (-> dbeta, dgamma, BatchNorm coefficients): g and ysel read once, dzs written
 * once (six torch ops = twelve passes otherwise).  Co in {64, 128, 256}; 16-byte aligned.  Deterministic. */
int fpsg_edgeconv_prep_blocks(long rows);
/* The per-channel scalar work between them, one launch each: fpsg_edgeconv_stats_finalize turns the forward kernel's
 * partial sums (count = B*N*k edge activations) into chan [4][Co] = (gamma*rstd, beta - mean*gamma*rstd, mean, rstd) and
 * updates the running statistics as nn.BatchNorm2d does (training = 0: chan from the running statistics);
 * fpsg_edgeconv_bwd_finalize turns fpsg_edgeconv_bwd_prep's partial sums into dgamma, dbeta and coef [3][Co] of
 * fpsg_edgeconv_bwd (zeros in eval mode).  fp64 sums in block order. */
int fpsg_edgeconv_stats_finalize(const float* part, int blocks, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var, float momentum, float eps, double count, int Co,
                                 int training, float* chan, fpsg_stream_t stream);
/* The same with the partial rows summed in two stages (round 4): slice sums over whole coalesced row pieces by ~256-512
 * workgroups into ws (fpsg_edgeconv_stats_ws_floats(blocks, Co) floats, 8-byte aligned: [Z][2 Co] doubles), then one wave per
 * channel.  Deterministic; equal to the one-launch form up to the order of its fp64 sums.  ws NULL, eval mode or fewer than
 * 256 rows: the one-launch form. */
size_t fpsg_edgeconv_stats_ws_floats(int blocks, int Co);
int fpsg_edgeconv_stats_finalize_ws(const float* part, int blocks, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, double count,
                                    int Co, int training, float* chan, float* ws, fpsg_stream_t stream);
int fpsg_edgeconv_bwd_finalize(const float* part, int blocks, const float* chan, double count, int Co, int training,
                               float* dgamma, float* dbeta, float* coef, fpsg_stream_t stream);
int fpsg_edgeconv_act(const float* ysel, const float* scale, const float* shift, float slope, long rows, int Co,
                      float* out, fpsg_stream_t stream);
int fpsg_edgeconv_bwd_prep(const float* g, const float* ysel, const float* scale, const float* shift, float slope,
                           long rows, int Co, float* dzs, float* part, fpsg_stream_t stream);

/* ---- K2b: soft-min of the Sinkhorn loop ---------------------------------------------
 * The operator under neuralnet_pytorch.metrics.emd_loss(sinkhorn=True) = geomloss.SamplesLoss()
 * (the form src/models/utils.py:12-13 actually calls): with cost |x-y|^2 / 2,
 *   out[b,i] = -eps * log sum_j exp( h[b,j] - |x_i - y_j|^2 / (2 eps) )
 * x [B,N,3], y [B,M,3], h [B,M] (log-weights + dual potential / eps), out [B,N].
 * No [B,N,M] matrix is formed.  Deterministic.
 */
int fpsg_softmin(const float* x, const float* y, const float* h, int B, int N, int M, float eps,
                 float* out, fpsg_stream_t stream);

/* The whole divergence of emd_wrapper (src/models/utils.py:12-13): the symmetric, annealed, debiased
 * Sinkhorn loop of geomloss.SamplesLoss("sinkhorn", p=2) between uniform clouds x [B,N,3], y [B,M,3]:
 *   duals a_x, b_x [N], a_y, b_y [M] start as the soft-mins of the log-weights at eps[0]; for every
 *   eps of the schedule the four soft-mins (h = log-weight + dual * (1/eps)) are evaluated from the
 *   previous duals and averaged in, new = (old + softmin)/2; one last un-averaged evaluation at
 *   eps[n-1];  out[b] = mean_i (b_x - a_x) + mean_j (a_y - b_y).
 * ONE launch per schedule entry (the four soft-mins side by side), n_eps + 3 launches in all.
 * eps_host: the schedule as n_eps HOST floats (geomloss: diameter^2, then diameter^2 * scaling^2k
 * down to blur^2, then blur^2); ws: fpsg_sinkhorn_workspace_floats(B,N,M) device floats.  Deterministic. */
size_t fpsg_sinkhorn_workspace_floats(int B, int N, int M);
int fpsg_sinkhorn_divergence(const float* x, const float* y, int B, int N, int M,
                             const float* eps_host, int n_eps, float* out, float* ws,
                             fpsg_stream_t stream);

/* ---- K19: the gradient of that divergence --------------------------------------------
 * What geomloss.SamplesLoss("sinkhorn") returns from backward(): NOT a backward pass through the loop.  geomloss runs
 * the annealing loop without autograd and then evaluates the final extrapolation with autograd on and three things
 * held as constants: the duals, the summed cloud of every soft-min, and the diameter with its schedule.  With
 * C(u,v) = |u-v|^2 / 2, e = eps[n_eps-1], (a_x, b_x, a_y, b_y) the duals in front of the final extrapolation and
 * w_ij = softmax_j( h_j - C(x_i, y_j) / e ):
 *   d out[b] / d x_i = ( D_xx(i) - D_xy(i) ) / N
 *       D_xy(i) = sum_j w_ij (y_j - x_i),  h_j = -log M + a_y[j] / e    (the weights of  b_x <- softmin over y)
 *       D_xx(i) = sum_k w_ik (x_k - x_i),  h_k = -log N + a_x[k] / e    (the weights of  a_x <- softmin over x)
 *   d out[b] / d y_j = ( D_yy(j) - D_yx(j) ) / M
 *       D_yx(j): owners y, summed cloud x, h_i = -log N + b_x[i] / e
 *       D_yy(j): owners y, summed cloud y, h_l = -log M + b_y[l] / e
 * -- each from the same soft-min, over the same summed cloud and the same h, as the final extrapolation evaluates.
 * The last launch of the call is that extrapolation with three more running sums per owner (the displacements
 * y_j - x_i, not barycentres: at e = blur^2 the xx weights sit on the point itself); one small launch forms the two
 * differences.  No [B,N,M] tensor, no atomics: bitwise reproducible, and the gradient of out(x, x) is exactly 0.
 *
 * out [B]: bit-identical to fpsg_sinkhorn_divergence for the same inputs and schedule.  gx [B,N,3], gy [B,M,3]: either
 * may be NULL, and its two soft-mins then skip the displacement sums.  ws: fpsg_sinkhorn_grad_workspace_floats(B,N,M)
 * device floats.  Argument checks, error codes and limits as fpsg_sinkhorn_divergence (FPSG_E_ALIGN for a misaligned
 * gx / gy).  n_eps + 4 launches; only enqueues (eps_host is read at call time: capturable in a graph). */
size_t fpsg_sinkhorn_grad_workspace_floats(int B, int N, int M);
int fpsg_sinkhorn_divergence_grad(const float* x, const float* y, int B, int N, int M,
                                  const float* eps_host, int n_eps, float* out,
                                  float* gx /*[B,N,3] or NULL*/, float* gy /*[B,M,3] or NULL*/,
                                  float* ws, fpsg_stream_t stream);

/* ---- K9: first layer of the decoder's patch MLPs ------------------------------------------
 * Replaces, per decode, the 16 x [conv1 (1539 -> 1539, 1x1) + BatchNorm1d + ReLU] of
 * PrimitiveNode.forward (src/models/point_cloud_net.py:76-80) applied to cat(x.repeat, patch points)
 * (src/models/point_cloud_net.py:105-110), in the split form  h[g,d,b,q] = hlat[g,d,b] + w[g,d,wofs:wofs+3] . pts[g,:,b,q]
 * with hlat = W[:, :L] x + bias computed by the caller (one GEMM per patch).  G patches, D channels, B clouds,
 * P points per patch (4 x a power of two, <= 256; B*P <= 8192).  w [G,D,ldw] is the stacked conv1 weight.
 *   fwd: out [G,D,B*P] = relu(BN(h)); statistics per (g,d) over the B*P values (training) or the given running
 *        statistics; chan [4][G*D] = (scale, shift, mean, rstd) for the backward; batch_mean /
 *        batch_var_unbiased [G*D] optional (training).  The pre-BatchNorm tensor is never stored.
 *   bwd: from dout [G,D,B*P]: dhlat [G,D,B] (gradient of the latent GEMM's output), the three point columns of
 *        dw (same layout / ldw / wofs as w; other columns untouched), dpts_part [G, fpsg_dec1_tiles(D), 3, B*P]
 *        (partial sums over channel tiles; the caller adds them up), dgamma, dbeta [G*D].
 * pts, out, dout 16-byte aligned.  Deterministic.
 * A workgroup keeps the patch's points and its 32 latent rows in LDS: 4 (3 B P + 32 B) bytes, the backward 24576 more.
 * Beyond the 163840 bytes of a CU (many small clouds: P = 16 from B = 436 in the backward, P = 4 from B = 931 in the
 * forward) the entry points answer FPSG_E_LIMIT.  fpsg_dec1_fits(B, P, bwd) is that shape check alone (P, B*P and
 * the LDS of the forward, bwd = 0, or the backward): 1 when a call of these sizes would pass it, else 0. */
int fpsg_dec1_tiles(int D);
int fpsg_dec1_fits(int B, int P, int bwd);
int fpsg_dec1_fwd(const float* hlat, const float* w, int ldw, int wofs, const float* pts,
                  const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                  int G, int D, int B, int P, int training, float eps, float* out, float* chan,
                  float* batch_mean, float* batch_var_unbiased, fpsg_stream_t stream);
int fpsg_dec1_bwd(const float* dout, const float* hlat, const float* w, int ldw, int wofs, const float* pts,
                  const float* chan, int G, int D, int B, int P, int training, float* dhlat, float* dw,
                  float* dpts_part, float* dgamma, float* dbeta, fpsg_stream_t stream);

/* The same with row strides: pts rows ld_pts apart, out / dout rows ld_out / ld_dout apart (multiples of 4, >= B*P),
 * hlat / dhlat rows ld_hlat apart (>= B) --
 * a call then owns a column range of tensors that hold several decodes side by side (an episode's query and support
 * decodes share every GEMM after this layer).  accumulate != 0: dw's point columns, dgamma and dbeta are added to the
 * buffers' contents (the second call of a pair) instead of overwriting them. */
int fpsg_dec1_fwd_ld(const float* hlat, int ld_hlat, const float* w, int ldw, int wofs, const float* pts, int ld_pts,
                     const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     int G, int D, int B, int P, int training, float eps, float* out, int ld_out, float* chan,
                     float* batch_mean, float* batch_var_unbiased, fpsg_stream_t stream);
int fpsg_dec1_bwd_ld(const float* dout, int ld_dout, const float* hlat, int ld_hlat, const float* w, int ldw, int wofs,
                     const float* pts, int ld_pts, const float* chan, int G, int D, int B, int P, int training,
                     int accumulate, float* dhlat, float* dw, float* dpts_part, float* dgamma, float* dbeta,
                     fpsg_stream_t stream);

/* ---- K5: BatchNorm fused with its activation (training and eval mode) -------------------
 * Replaces the BatchNorm{1,2}d + ReLU / LeakyReLU module pairs of the reference networks
 * (src/models/image_net.py:14 VGG16-BN trunk; src/pointnet/model.py:30-44,220-233;
 * src/models/point_cloud_net.py:52-54,76-79) on [N,C,L]-contiguous fp32 tensors; statistics
 * per channel over (N,L).  act: 0 none, 1 ReLU, 2 LeakyReLU(slope).
 *   fwd: y = act((x-mean)*rstd*gamma+beta); chan [4][C] receives (scale, shift, mean, rstd) for
 *        the backward; training != 0: batch statistics; running_mean / running_var [C] (optional)
 *        are then updated in place, running <- (1-momentum)*running + momentum*batch (unbiased
 *        variance), unless momentum < 0; batch_mean / batch_var_unbiased [C] are optional outputs
 *        for a caller with its own update rule.  training == 0: running_mean/var are the statistics.
 *        training == 2 (fpsg_bn_act_fwd, fpsg_bn_act_pool_fwd, fpsg_bn_act_max_fwd): evaluation mode with chan ALREADY
 *        holding the coefficients -- the caller got them once from fpsg_bn_stats(training = 0) for a block of calls in
 *        which the running statistics do not change (the evaluation loop, src/evaluate_Network.py:107-118); saves the
 *        coefficient launch of every layer and item.
 *   bwd: dx [N,C,L], dgamma [C], dbeta [C] from x, dy and chan (the activation mask is
 *        re-derived from x); coef [3][C] scratch.
 * pre_bias [C] (optional, NULL = none): the bias of the convolution in front of the BatchNorm
 * (the Conv2d/Conv1d + BatchNorm + ReLU triples of image_net.py:14, pointnet/model.py:30-44);
 * x is then the bias-free convolution output and the op is act(BN(x + pre_bias[c])), with
 * fl(x + pre_bias) formed in registers; bwd additionally returns dpre_bias[c] = sum over (n,l)
 * of dx (optional, NULL = skip) -- the bias gradient autograd would reduce from dx.
 * ws: fpsg_bn_workspace_floats(N,C,L) floats.  x, y, dy, dx 16-byte aligned.  Deterministic.
 */
size_t fpsg_bn_workspace_floats(int N, int C, int L);
int fpsg_bn_act_fwd(const float* x, const float* pre_bias, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, int N, int C, int L, int training,
                    float eps, int act, float slope, float* y, float* chan, float* batch_mean,
                    float* batch_var_unbiased, float* ws, fpsg_stream_t stream);
/* Statistics half of fpsg_bn_act_fwd alone: chan [4][C] (scale, shift, mean, rstd) from the batch (training; running
 * statistics updated as there) or from the running statistics (eval); nothing is applied or written besides.
 * parts (optional, training): partial sums [C][n_parts][2] = (sum(x + pre_bias), sum((x + pre_bias)^2)) that the
 * producing convolution's epilogue accumulated (fpsg_wino_output_transform_stats, fpsg_wino_conv_fused_stats):
 * the pass over x is skipped and only the fp64 finalize runs (ws may then be NULL). */
int fpsg_bn_stats(const float* x, const float* pre_bias, const float* gamma, const float* beta,
                  float* running_mean, float* running_var, float momentum, int N, int C, int L, int training,
                  float eps, float* chan, float* batch_mean, float* batch_var_unbiased, float* ws,
                  const float* parts, int n_parts, fpsg_stream_t stream);
int fpsg_bn_act_bwd(const float* x, const float* pre_bias, const float* dy, const float* chan, int N, int C,
                    int L, int training, int act, float slope, float* dx, float* dgamma, float* dbeta,
                    float* dpre_bias, float* coef, float* ws, fpsg_stream_t stream);
/* The sums + coefficient half of fpsg_bn_act_bwd alone: dgamma, dbeta, coef [3,C] = (k1, k2, k3) of
 * dx = k1 dz + k2 (x + pre_bias) + k3 -- for a consumer that forms dx itself while reading x and dy
 * (fpsg_conv_first_dw_fold).  N * L above the small-tensor limit (16384) only; ws as fpsg_bn_act_bwd. */
int fpsg_bn_act_bwd_coef(const float* x, const float* pre_bias, const float* dy, const float* chan, int N, int C,
                         int L, int training, int act, float slope, float* dgamma, float* dbeta, float* coef,
                         float* ws, fpsg_stream_t stream);
/* Training-mode K5 over column segments of C rows that lie ld elements apart (x, y, dy, dx share the layout): segment i
 * = the elements seg_off[i] .. seg_off[i] + seg_len[i] - 1 of every row is one BatchNorm call (one reference
 * BatchNorm1d call per patch and decode, src/models/point_cloud_net.py:76-80): own statistics, one launch for all
 * segments.  nseg <= 4, seg_len <= 16384, ld and seg_off multiples of 4 (host arrays), segments disjoint.
 *   fwd: y = act(BN(x + pre_bias)); chan [nseg][4][C]; stats [nseg][2][C] (optional): batch mean, unbiased batch variance.
 *   bwd: dx; dgamma, dbeta, dpre_bias (optional) [nseg][C] -- the caller adds the segments (the affine parameters are
 *        shared).  Columns outside every segment are neither read nor written. */
int fpsg_bn_act_rows_fwd(const float* x, int ld, const int* seg_off, const int* seg_len, int nseg,
                         const float* pre_bias, const float* gamma, const float* beta, int C, float eps, int act,
                         float slope, float* y, float* chan, float* stats, fpsg_stream_t stream);
int fpsg_bn_act_rows_bwd(const float* x, int ld, const int* seg_off, const int* seg_len, int nseg,
                         const float* pre_bias, const float* dy, const float* chan, int C, int act, float slope,
                         float* dx, float* dgamma, float* dbeta, float* dpre_bias, fpsg_stream_t stream);
/* fpsg_bn_act_bwd with the two sums per channel delivered by the kernel that produced dy
 * (fpsg_wino_output_transform_bwd_stats): parts [C][n_parts][2].  ws may be NULL unless dpre_bias is wanted. */
int fpsg_bn_act_bwd_parts(const float* x, const float* pre_bias, const float* dy, const float* chan, int N,
                          int C, int L, int training, int act, float slope, float* dx, float* dgamma,
                          float* dbeta, float* dpre_bias, float* coef, float* ws, const float* parts,
                          int n_parts, fpsg_stream_t stream);

/* K5 followed by MaxPool2d(kernel 2, stride 2): the conv + BatchNorm + ReLU + max-pool groups
 * that end the five stages of the VGG16-BN trunk (src/models/image_net.py:14).  x [N,C,H,W]
 * (H, W even), y_pooled / dy_pooled [N,C,H/2,W/2].  The forward writes only the pooled
 * tensor; the backward re-derives each window's activations and arg-max from x (scan order
 * (h,w), first strictly greater or NaN wins, as torch's max_pool2d), so neither the
 * full-resolution activation, nor pooling indices, nor the scattered gradient exist in HBM.
 * Other arguments as fpsg_bn_act_fwd / _bwd; ws: fpsg_bn_pool_workspace_floats(N,C,H,W); parts / n_parts as
 * fpsg_bn_stats (statistics delivered by the producing convolution).
 */
size_t fpsg_bn_pool_workspace_floats(int N, int C, int H, int W);
int fpsg_bn_act_pool_fwd(const float* x, const float* pre_bias, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, int N, int C, int H, int W,
                         int training, float eps, int act, float slope, float* y_pooled, float* chan,
                         float* batch_mean, float* batch_var_unbiased, float* ws, const float* parts, int n_parts,
                         fpsg_stream_t stream);
int fpsg_bn_act_pool_bwd(const float* x, const float* pre_bias, const float* dy_pooled, const float* chan,
                         int N, int C, int H, int W, int training, int act, float slope, float* dx,
                         float* dgamma, float* dbeta, float* dpre_bias, float* coef, float* ws,
                         fpsg_stream_t stream);

/* K5 followed by the max over the row: max_l act(BN(x + pre_bias))[n,c,l] -> out [N,C], the
 * BatchNorm (+ReLU) + torch.max(x, 2) tails of PointNet's shared MLPs (src/pointnet/model.py:35-37,
 * 222-224).  act and BN are monotone, so only each row's extreme of x is normalised: the forward
 * is one read of x (no normalised tensor is written), idx [N,C] receives the selected position
 * (first arg-max of x where scale >= 0, first arg-min otherwise); the backward takes gout [N,C],
 * and is one read + one write (dx).  Other arguments as fpsg_bn_act_fwd / _bwd;
 * ws: fpsg_bn_max_workspace_floats(N,C,L).  fpsg_bn_max_dz_offset(N,C,L): where, in floats from the start of that
 * workspace, fpsg_bn_act_max_bwd_coef leaves dz [N,C] (the gradient at the selected positions, in front of the
 * BatchNorm) for fpsg_max_bwd_gather / _prep / _scatter -- the workspace layout is the library's, not the caller's.
 */
size_t fpsg_bn_max_workspace_floats(int N, int C, int L);
size_t fpsg_bn_max_dz_offset(int N, int C, int L);
int fpsg_bn_act_max_fwd(const float* x, const float* pre_bias, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, int N, int C, int L, int training,
                        float eps, int act, float slope, float* out, int32_t* idx, float* chan, float* batch_mean,
                        float* batch_var_unbiased, float* ws, fpsg_stream_t stream);
int fpsg_bn_act_max_bwd(const float* x, const float* pre_bias, const float* gout, const int32_t* idx,
                        const float* chan, int N, int C, int L, int training, int act, float slope, float* dx,
                        float* dgamma, float* dbeta, float* dpre_bias, float* coef, float* ws, fpsg_stream_t stream);
/* The coefficient pass of fpsg_bn_act_max_bwd alone (no dense dx): dgamma, dbeta, coef [3][C] = k1, k2, k3 of
 * dx'[n,c,l] = k1_c dz[n,c] [l = idx[n,c]] + k2_c (x[n,c,l] + pre_bias_c) + k3_c, and dz [N,C] left in ws at float offset
 * C*128 + N*C*ceil(L/4096)*4.  ws: fpsg_bn_max_workspace_floats(N,C,L) floats. */
int fpsg_bn_act_max_bwd_coef(const float* x, const float* pre_bias, const float* gout, const int32_t* idx,
                             const float* chan, int N, int C, int L, int training, int act, float slope,
                             float* dgamma, float* dbeta, float* coef, float* ws, fpsg_stream_t stream);

/* ---- K5m: backward of conv1x1 -> BatchNorm (+ReLU) -> max over the points without the dense gradient ----------
 * (PointNet's last shared layer, src/pointnet/model.py:35-37, 222-224).  With the coefficients of
 * fpsg_bn_act_max_bwd_coef the two GEMMs over the [B,C,L] gradient reduce to K x K algebra (library GEMMs on the
 * caller's side, fpsg_amd/fused_bn.py) plus these two passes.  a [B,K,L] the layer's input, W [C,K], idx [B,C] the
 * selected point of every row, dz [B,C].
 *   fpsg_max_bwd_gather : S[c,k] = sum_b dz[b,c] a[b,k,idx[b,c]]            (ascending b; L % 4 == 0, L <= 2048)
 *   fpsg_max_bwd_scatter: da[b,k,l] += v[k] + sum_{c: idx[b,c] = l} (k1[c] dz[b,c]) W[c,k]   (ascending c; K <= 128,
 *                         L < 65407; ws: fpsg_max_bwd_scatter_workspace_floats(B,C,L) floats of caller scratch)
 * Deterministic (no float atomics). */
int fpsg_max_bwd_gather(const float* a, const float* dz, const int32_t* idx, int B, int K, int C, int L, float* S,
                        float* spart /* [B,K] row sums of a, or NULL */, fpsg_stream_t stream);
/*   fpsg_max_bwd_prep   : Wk = diag(k2) W, u = k2 pb + k3, dpre_bias = k1 sum_b dz + (k2 mean + k3) B L, and (spart, s
 *                         given) s[k] = sum_b spart[b,k], spart [B,K] = the row sums of a                 (one launch)
 *   fpsg_max_bwd_dw     : dw = k1 S + k2 (WG + pb s^T) + k3 s^T; WG = NULL (eval mode): dw = k1 S */
int fpsg_max_bwd_prep(const float* W, const float* coef, const float* pre_bias, const float* mean, const float* dz,
                      const float* spart, int B, int K, int C, int L, float* Wk, float* u, float* dpre_bias, float* s,
                      fpsg_stream_t stream);
int fpsg_max_bwd_dw(const float* S, const float* WG, const float* coef, const float* pre_bias, const float* s, int B,
                    int K, int C, float* dw, fpsg_stream_t stream);
size_t fpsg_max_bwd_scatter_workspace_floats(int B, int C, int L);
int fpsg_max_bwd_scatter(float* da, const float* W, const float* k1, const float* dz, const int32_t* idx, const float* v,
                         int B, int K, int C, int L, float* ws, fpsg_stream_t stream);


/* ---- K6: Winograd F(m x m, 3x3) transforms (m = 2 or 4) for the deep 3x3 convolutions -------
 * Replaces, together with the caller's fp32 batched GEMM (hipBLASLt, MFMA), the library
 * convolution under the Conv2d(3x3, padding 1) layers of torchvision's vgg16_bn.features that
 * src/models/image_net.py:14 instantiates (forward :21-24, full backward: SURVEY.md F9).
 * With A = m + 2 and P = N*(H/m)*(W/m) tiles (tile p = (n*(H/m) + th)*(W/m) + tw; H, W multiples
 * of m):
 *   y  = conv(x, w):           U = filter(w, flip 0) [A*A,K,C];  V = input(x) [A*A,C,P];
 *                              M[xi] = U[xi] V[xi] [A*A,K,P];     y = output(M)
 *   dx = conv(dy, rot180 w^T): U' = filter(w, flip 1) [A*A,C,K]; V' = input(dy) [A*A,K,P];
 *                              M'[xi] = U'[xi] V'[xi] [A*A,C,P]; dx = output(M')
 *   dw:                        dM = grad_output(dy) [A*A,K,P];   dU[xi] = dM[xi] V[xi]^T [A*A,K,C];
 *                              dw = filter_grad(dU)
 * m = 2: 2.25x fewer multiplications than the direct form, fp32 error a few ulp; m = 4: 4x fewer,
 * error ~1e-5 of the output scale (transform constants up to 8 and 1/24).  All tensors fp32,
 * contiguous, caller-allocated; image tensors 16-byte aligned.  Deterministic.
 * ldp (round 5): the ROW STRIDE of the transform-domain tensors V / M / dM in floats -- [A*A][channels][ldp], tile p of a
 * row at offset p -- 0 (= P, dense) or any value >= P.  P is 29008 / 7252 / 1813 / 592 at the trunk's shapes: never a
 * whole number of 128-byte lines (1813 is odd), so dense rows make every row piece a GEMM tile reads or writes share
 * its first and last line with the neighbouring tile; with ldp = P rounded up to 32 floats the library's products run
 * 4-13 % faster (profiles/r05/wino_row_stride.txt).  The transforms that WRITE a transform-domain tensor fill the pad
 * columns P .. ldp-1 with zeros (the products may then simply run over ldp columns: a zero column adds nothing to the
 * weight gradient's reduction); the output transforms never read them.
 */
int fpsg_wino_input_transform(int m, const float* x, int N, int C, int H, int W, float* V, long ldp,
                              fpsg_stream_t stream);
int fpsg_wino_output_transform(int m, const float* M, int N, int K, int H, int W, float* y, long ldp,
                               fpsg_stream_t stream);
/* The same, also accumulating the statistics of the BatchNorm that follows the convolution
 * (nn.Conv2d -> nn.BatchNorm2d of image_net.py:14): parts [K][fpsg_wino_stats_parts(m,N,H,W)][2] =
 * (sum(y + bias[k]), sum((y + bias[k])^2)) per workgroup of 256 tiles (bias optional: the convolution's bias, which K5
 * adds inside the BatchNorm); fpsg_bn_stats / fpsg_bn_act_pool_fwd take them instead of reading y again.  Deterministic. */
int fpsg_wino_stats_parts(int m, int N, int H, int W);
int fpsg_wino_output_transform_stats(int m, const float* M, int N, int K, int H, int W, float* y, const float* bias,
                                     float* parts, long ldp, fpsg_stream_t stream);
/* The output transform of a DATA-GRADIENT convolution whose result is the gradient of relu(bn(xpre + pre_bias)):
 * besides y it delivers the two sums BatchNorm's backward starts from -- sum(dz) and sum(dz * (x - mean) * rstd) with
 * dz = y * [fma(x, scale, shift) > 0], x = xpre + pre_bias[k] -- per output channel and workgroup into
 * parts [K][fpsg_wino_stats_parts(m,N,H,W)][2] (deterministic), in the arithmetic of fpsg_bn_act_bwd's own pass.
 * xpre [N,K,H,W]: the pre-BatchNorm tensor; chan [4][K]: scale, shift, mean, rstd (fpsg_bn_stats / _act_fwd).
 * fpsg_bn_act_bwd_parts then skips its pass over (x, dy). */
int fpsg_wino_output_transform_bwd_stats(int m, const float* M, int N, int K, int H, int W, float* y,
                                         const float* xpre, const float* pre_bias, const float* chan,
                                         float* parts, long ldp, fpsg_stream_t stream);
int fpsg_wino_grad_output_transform(int m, const float* dy, int N, int K, int H, int W, float* dM, long ldp,
                                    fpsg_stream_t stream);
/* Both transforms of an output gradient dy [N,K,H,W] in ONE pass (round 4): V = B^T d B of its 6x6 (4x4) patches -- the
 * "input" transform of the data gradient's convolution -- and dM = A dy A^T of its tiles -- the weight gradient's -- the
 * tile being the patch's interior.  V, dM [A*A, K, P]; values bit-identical to fpsg_wino_input_transform(dy) and
 * fpsg_wino_grad_output_transform(dy); one read of dy instead of two. */
int fpsg_wino_grad_transforms(int m, const float* dy, int N, int K, int H, int W, float* V, float* dM, long ldp,
                              fpsg_stream_t stream);
int fpsg_wino_filter_transform(int m, const float* w, int K, int C, int flip_transpose, float* U,
                               fpsg_stream_t stream);
/* Every filter transform of an optimizer step in one launch (the weights change once per step): jobs [n_jobs][6]
 * int64 in DEVICE memory -- w pointer [K][C][3][3], U pointer (layout of fpsg_wino_filter_transform), K, C,
 * 2*m + flip_transpose, first workgroup of the job -- with the jobs' workgroups (256 filters each, ceil(K*C/256) per
 * job) numbered consecutively; total_blocks = their sum.  Same arithmetic per filter as the single form. */
int fpsg_wino_filter_transform_batch(const int64_t* jobs, int n_jobs, long total_blocks, fpsg_stream_t stream);
int fpsg_wino_filter_grad_transform(int m, const float* dU, int K, int C, float* dw, fpsg_stream_t stream);

/* ---- K10 (round 5, opt-in: FPSG_GEMM_SPLIT=1): batched fp32 GEMM on the bf16 matrix pipe, operands split three ways ----
 * Replaces the library fp32 GEMMs (torch.bmm -> rocBLAS / hipBLASLt, fp32 MFMA at 1/16 of the bf16 rate) behind the
 * Winograd-domain products of the trunk's 3x3 convolutions (torchvision vgg16_bn.features built at
 * src/models/image_net.py:14, run at src/models/image_net.py:21-24).
 *   transB = 0:  C[b] [M x N] = A[b] [M x K] . B[b] [K x N]     (forward / data gradient: U[xi] . V[xi])
 *   transB = 1:  C[b] [M x N] = A[b] [M x K] . B[b]^T, B [N x K] (weight gradient: dM[xi] . V[xi]^T; the reduction is
 *                split over workgroups, partial slabs in ws, added in a fixed order: deterministic)
 * Row-major, leading dimensions lda / ldb / ldc and batch strides sA / sB / sC in floats.  Every fp32 operand x enters as
 * bf16(x) + bf16(x - x1) + bf16(x - x1 - x2) (an exact split) and the six products of order <= 2^-18 are accumulated in
 * fp32 by v_mfma_f32_32x32x16_bf16: fp32-grade results (error against float64: profiles/r05/), not the library's bits.
 * variant: -1 automatic; else tile + 10 * splits (0-999) with splits 0 = automatic, 1-99 = that many ranges of the
 * reduction (transB = 1), and tile 0 = 256x256x16, 1 = 256x128x32, 2 = 128x128x16, 3 = 128x256x16, 4 / 5 / 6 = tiles
 * 0 / 2 / 3 with the split placed among the MFMAs (5 is what -1 picks but for long weight-gradient reductions: 0),
 * 7 = 256x128x16 in the same form.  Every other id (tile 8 or 9, anything >= 1000 or below -1) is refused on the host
 * with FPSG_E_SHAPE, and fpsg_gemm_split_workspace_floats returns 0 for it.
 * ws: fpsg_gemm_split_workspace_floats(...) floats (0 when the reduction is not split; then ws may be NULL); a split
 * reduction needs a dense output (ldc == N, sC == M*N).  One batch entry of each matrix must stay below 2 GiB.
 * Both forms are deterministic (no float atomics). */
size_t fpsg_gemm_split_workspace_floats(int batch, int M, int N, int K, int transB, int variant);
int fpsg_gemm_split(const float* A, const float* B, float* C, int batch, int M, int N, int K, int lda, int ldb, int ldc,
                    long sA, long sB, long sC, int transB, int variant, float* ws, size_t ws_floats,
                    fpsg_stream_t stream);

/* K10 with the A operand split once (the transformed filters: constant over an optimizer step).  fpsg_gemm_split_pack_a writes
 * A [batch][M][K] (row-major, lda, batch stride sA) as three bf16 planes in the layout of the GEMM's LDS image, zero-padded
 * (fpsg_gemm_split_packed_a_bytes bytes, 16-byte aligned; about 1.5x the fp32 matrix); fpsg_gemm_split_nn_packed computes
 * C[b] [M x N] = A[b] . B[b] [K x N] with A brought in by LDS-DMA and only B split on the way into LDS: the same values as
 * fpsg_gemm_split(transB = 0), bit for bit.  variant (the same for the three calls): -1 / 0 = 256 x 128 x 16 tiles, two
 * workgroups per CU; 1 = 256 x 256 x 16; 2 = 128 x 128 x 16; 3 = the tiled kernel of fpsg_gemm_split (tile 5) with A staged
 * through registers from the image packed for 2.  Every other id: FPSG_E_SHAPE (0 bytes from fpsg_gemm_split_packed_a_bytes). */
size_t fpsg_gemm_split_packed_a_bytes(int batch, int M, int K, int variant);
int fpsg_gemm_split_pack_a(const float* A, int batch, int M, int K, int lda, long sA, int variant, void* Ap,
                           fpsg_stream_t stream);
int fpsg_gemm_split_nn_packed(const void* Ap, const float* B, float* C, int batch, int M, int N, int K, int ldb, int ldc,
                              long sB, long sC, int variant, fpsg_stream_t stream);

/* The same product as fpsg_gemm_split_nn_packed (Ap packed with variant 0 or 1: 256-row tiles) as ONE persistent launch:
 * a workgroup per CU walks an equal share of the flattened (batch, row tile, column) space, the load / split / MFMA
 * pipeline runs across tile boundaries (no per-tile launch, prologue or drain; 1044 tiles on 256 CUs cost 4.08 rounds, not
 * 5).  Same values as fpsg_gemm_split_nn_packed bit for bit.  variant: -1 / 0 = 256 columns per tile, 1 = 128;
 * 6 / 12 = the form with specialised waves (4 waves only multiply, 4 only stage: LDS-DMA of both operands, the split of B
 * from LDS), 256 x 128 tiles, 12 with staggered first pieces; 13 / 14 = the same with 128 x 128 tiles and two workgroups
 * per CU (Ap packed with variant 2).  6 and 12-14 move B rows by 16-byte DMA: B, ldb and sB aligned to 4 floats
 * (FPSG_E_SHAPE otherwise).  Every other id is refused on the host with FPSG_E_SHAPE (2-5 and 7-11 once named
 * measurement builds that computed wrong results by design: removed).  Measured: none of the persistent forms beats the
 * tiled kernel (profiles/r05/gemm_split_ablation.txt); they are kept as measured evidence and are not on any product
 * path.  B below 4 GiB in total, one C matrix and the packed A below 2 GiB. */
int fpsg_gemm_split_nn_persistent(const void* Ap, const float* B, float* C, int batch, int M, int N, int K, int ldb, int ldc,
                                  long sB, long sC, int variant, fpsg_stream_t stream);

/* ---- K11: batched fp32 GEMM on the fp32 matrix pipe, hand-written (round 5) -------------------------------------------
 * C[b] [M x N] = A[b] [M x K] . B[b] [K x N], row-major, leading dimensions / batch strides in floats: the product
 * torch.bmm hands to rocBLAS / hipBLASLt for the Winograd-domain GEMMs of torchvision vgg16_bn.features
 * (src/models/image_net.py:14,21-24) and the decoder's wide layers (src/models/point_cloud_net.py:66-79), with the same
 * arithmetic class (v_mfma_f32_32x32x2_f32: fp32 products, fp32 accumulation; the order of the sum differs from the
 * library's, so results agree to fp32 round-off, not bit for bit).  One persistent launch: a workgroup per CU walks an
 * equal share of the flattened (batch, row tile, column) space; four waves stage both operands by LDS-DMA, four multiply.
 * K, lda, ldb, sA, sB multiples of 4 floats, A and B 16-byte aligned (FPSG_E_ALIGN otherwise: the caller then takes the
 * library GEMM); A and B below 4 GiB each in total, one C matrix below 2 GiB.  variant: 0 = 256 x 128 tiles, one workgroup per CU;
 * 2 (and -1) = 128 x 128 tiles, two per CU; 1 / 3 = 0 / 2 with staggered first pieces; every other id: FPSG_E_SHAPE.
 * Deterministic. */
int fpsg_gemm_f32_nn(const float* A, const float* B, float* C, int batch, int M, int N, int K, int lda, int ldb, int ldc,
                     long sA, long sB, long sC, int variant, fpsg_stream_t stream);

/* K6 in one kernel for 64 input channels (F(4x4,3x3); conv1_2 / conv2_1 of the trunk and their data
 * gradients): y [N,K,H,W] = conv(x [N,64,H,W], w) from U = fpsg_wino_filter_transform(4, w, ...)
 * [36,K,64]; input transform, the 36 MFMA products and the output transform stay on chip -- with 64
 * channels the separate GEMM is bound by the traffic of V and M (2 x 2.25 x the image tensor each
 * way).  C must be 64, K a multiple of 16, H and W multiples of 4; x, y, U 16-byte aligned; x below 4 GiB
 * (32-bit lane offsets; FPSG_E_LIMIT otherwise -- the caller then takes the three-kernel form).
 */
int fpsg_wino_conv_fused(const float* x, const float* U, int N, int C, int K, int H, int W, float* y,
                         fpsg_stream_t stream);

/* fpsg_wino_conv_fused / _act (chan = NULL: the plain form) also accumulating the statistics of the BatchNorm that
 * follows this convolution: parts [K][fpsg_wino_conv_fused_parts(N,K,H,W)][2] = (sum(y + out_bias[k]),
 * sum((y + out_bias[k])^2)) per workgroup (out_bias optional), taken by fpsg_bn_stats / fpsg_bn_act_pool_fwd instead of
 * reading y again.  Deterministic. */
int fpsg_wino_conv_fused_parts(int N, int K, int H, int W);
int fpsg_wino_conv_fused_stats(const float* x, const float* chan, const float* pre_bias, const float* U, int N, int C,
                               int K, int H, int W, float* y, const float* out_bias, float* parts, fpsg_stream_t stream);

/* K6w: the WEIGHT gradient of the same convolutions (64 input channels) in one pass: dU [36,K,64] = sum over tiles of
 * (A dY A^T)[k] x (B^T d B)[c], both transform-domain operands formed in registers from dy [N,K,H,W] and the layer's
 * input x [N,64,H,W] (chan != NULL: x is the PRE-BatchNorm tensor and relu(fma(x + pre_bias[c], chan[c], chan[C+c]))
 * is what the convolution saw, as in fpsg_wino_conv_fused_act); dw = fpsg_wino_filter_grad_transform(4, dU).  Replaces
 * fpsg_wino_input_transform + fpsg_wino_grad_output_transform + the batched GEMM with the tile-long reduction.
 * H a multiple of 4, W of 16 (the four tiles of an MFMA step lie in one tile row); x, dy 16-byte aligned and below
 * 2 GiB each; ws: fpsg_wino_dw_fused_workspace_floats(N,K,H,W) floats (per-range partials, summed in a fixed order in
 * fp64).  Deterministic.
 */
size_t fpsg_wino_dw_fused_workspace_floats(int N, int K, int H, int W);
int fpsg_wino_dw_fused(const float* x, const float* chan, const float* pre_bias, const float* dy, int N, int C, int K,
                       int H, int W, float* dU, float* ws, fpsg_stream_t stream);

/* The same two entry points reading a PRE-BatchNorm tensor: the values fed to the transform are
 * relu(fma(x + pre_bias[c], chan[c], chan[C + c])) -- K5's apply arithmetic with chan = (scale, shift, ..) from
 * fpsg_bn_stats / fpsg_bn_act_fwd -- so that the BatchNorm + ReLU apply pass between two convolutions of a VGG
 * stage (conv -> BN -> ReLU -> conv, src/models/image_net.py:14) is folded into the second convolution's
 * load (one read + one write of the activation tensor less per layer).  pre_bias may be NULL. */
int fpsg_wino_input_transform_act(int m, const float* x, const float* chan, const float* pre_bias, int N, int C,
                                  int H, int W, float* V, long ldp, fpsg_stream_t stream);
int fpsg_wino_conv_fused_act(const float* x, const float* chan, const float* pre_bias, const float* U, int N, int C,
                             int K, int H, int W, float* y, fpsg_stream_t stream);

/* ---- K8: weight gradient of the first VGG convolution (3 -> 64 channels, 3x3, padding 1) ------
 * vgg16_bn.features[0] of src/models/image_net.py:14 in the backward of the train step:
 * dw [64,3,3,3] = sum over (n,h,w) of dy[n,k,h,w] * x[n,c,h+a-1,w+b-1], x [N,3,H,W], dy [N,64,H,W]
 * (W a multiple of 4, dy 16-byte aligned).  dy is read once (LDS-staged tiles feeding fp32 MFMA),
 * the workgroups' partial sums are reduced in a fixed order: HBM-bound, deterministic.
 * ws: fpsg_conv_first_dw_workspace_floats(N,H,W) floats.
 */
size_t fpsg_conv_first_dw_workspace_floats(int N, int H, int W);
int fpsg_conv_first_dw(const float* x, const float* dy, int N, int C, int K, int H, int W, float* dw, float* ws,
                       fpsg_stream_t stream);
/* The same weight gradient when dy is the BatchNorm + ReLU backward of the layer behind this convolution
 * (conv1_1 -> bn -> relu -> conv1_2 of src/models/image_net.py:14 in loss.backward()): instead of dy the call takes
 * the convolution's own output y [N,64,H,W], the gradient ga [N,64,H,W] of the activation relu(bn(y + pre_bias)), K5's
 * chan [4,64] (scale, shift, ..) and coef [3,64] (fpsg_bn_act_bwd_coef), and forms
 *   dy = k1 dz + k2 (y + pre_bias) + k3,  dz = ga * [(y + pre_bias) scale + shift > 0]
 * while it stages a tile (fpsg_bn_act_bwd's dx pass, bit for bit): K5's dx pass and its 475 MB dy (37 images at
 * 224 x 224) never exist.  Same result as fpsg_bn_act_bwd + fpsg_conv_first_dw, bit for bit. */
int fpsg_conv_first_dw_fold(const float* x, const float* y, const float* ga, const float* chan, const float* coef,
                            const float* pre_bias, int N, int C, int K, int H, int W, float* dw, float* ws,
                            fpsg_stream_t stream);
/* K8f: the forward of the same layer, y [N,64,H,W] = conv(x [N,3,H,W], w [64,3,3,3]), zero padding, no bias
 * (nn.Conv2d(3, 64, 3, padding=1) of vgg16_bn.features[0]; K5 adds the bias inside the BatchNorm).  Bound by the
 * write of y; per output the 27 taps are added in (c, a, b) order by an fma chain from 0.  parts (optional):
 * [64][fpsg_conv_first_parts(N,H,W)][2] partial sums of y + bias[k] (bias optional) and its square for the
 * BatchNorm that follows (fpsg_bn_stats with parts).  W a multiple of 4; x, y 16-byte aligned.  Deterministic.
 */
int fpsg_conv_first_parts(int N, int H, int W);
int fpsg_conv_first_fwd(const float* x, const float* w, int N, int C, int K, int H, int W, float* y, const float* bias,
                        float* parts, fpsg_stream_t stream);

/* ---- K7: Adam step over flat buffers ---------------------------------------------------------
 * Replaces torch.optim.Adam(lr, betas=(.9,.999)).step() of the train loop (src/trainNetwork.py:
 * 118-123, 144) when parameters, gradients and the two moments each live in one flat fp32 buffer
 * of n elements (fpsg_amd/optim.py): one 4-read / 3-write stream.  step = 1 for the first update
 * (bias corrections 1 - beta^step); grad_scale multiplies the gradient first (1/E for the mean
 * over the E episodes of a step).  amsgrad, weight decay and maximize are not part of the reference
 * configuration and not provided.  Buffers 16-byte aligned.
 */
int fpsg_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                   float beta1, float beta2, float eps, int step, float grad_scale, fpsg_stream_t stream);
/* The same step with the gradient left where autograd put it: segment s of the flat buffers is
 * [seg_off[s], seg_off[s+1]) (seg_off: nseg+1 int64 on the device, seg_off[0] = 0, seg_off[nseg] = n)
 * and its gradient is the contiguous fp32 tensor at grad_ptrs[s] (device array of nseg device
 * pointers; NULL = no gradient = zero).  Saves the gather of the gradients into a flat buffer when a
 * step is one episode on one rank (the reference's own loop, trainNetwork.py:140-148).  param, exp_avg and
 * exp_avg_sq 16-byte aligned (FPSG_E_ALIGN otherwise); the gradient tensors may start anywhere.
 */
int fpsg_adam_step_segments(float* param, const float* const* grad_ptrs, const long long* seg_off, int nseg,
                            float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                            float eps, int step, float grad_scale, fpsg_stream_t stream);
/* The gradient accumulation of a step of several episodes (optimizer.zero_grad() once, loss.backward() per
 * episode, trainNetwork.py:140-148) on the flat gradient buffer: flat[i] += the segment table's gradient
 * (accumulate = 1; segments without gradient untouched) or flat[i] = it (accumulate = 0: first episode, zeros where a
 * segment has none).  Same table format as fpsg_adam_step_segments; one stream at HBM rate.  flat 16-byte aligned.
 */
int fpsg_flat_accumulate_segments(float* flat, const float* const* grad_ptrs, const long long* seg_off, int nseg,
                                  size_t n, int accumulate, fpsg_stream_t stream);
/* The same for ntab (<= 8) tables at once, grad_ptrs [ntab][nseg]: flat (+)= g_0 + g_1 + ... added in table order -- the
 * fp32 sums of ntab consecutive fpsg_flat_accumulate_segments calls bit for bit, with flat read and written once (the
 * episodes of a step keep their gradient tensors until the step's last backward). */
int fpsg_flat_accumulate_tables(float* flat, const float* const* grad_ptrs, const long long* seg_off, int nseg, int ntab,
                                size_t n, int accumulate, fpsg_stream_t stream);

/* ---- K20: gradient-norm clipping folded into K7's factor ------------------------------------------
 * torch.nn.utils.clip_grad_norm_(params, max_norm) (2-norm, error_if_nonfinite=False) in front of the Adam step,
 * without a pass that rewrites the gradient and without a host read: one read of the gradient for the sum of its
 * squares, one finalize launch that leaves grad_scale * coef in device memory, and the _dscale forms of K7's entry
 * points, which take their factor from there.  The norm is that of grad_scale * grad, the gradient the update uses.
 *
 * Sum of squares (pinned: the order of every add depends on n alone, not on the device, the stream or the run):
 *   P = min(ceil((n/4 + 1) / 256), 4096) workgroups of 256 threads, T = 256 P threads; vector slot j holds the flat
 *   positions 4j .. 4j+3, slot n/4 the n % 4 tail padded with zeros.  Thread t takes the slots t, t + T, t + 2T, ..
 *   in that order; element e of a slot goes into the thread's accumulator e, a_e = fma(g, g, a_e) in fp64 from +0.0
 *   (the square of an fp32 value is exact in fp64).  The thread's value is (a_0 + a_1) + (a_2 + a_3); a wave's is the
 *   butterfly v += v[lane ^ 1], ^ 2, ^ 4, ^ 8, ^ 16, ^ 32; a workgroup's is (w_0 + w_1) + (w_2 + w_3) over its four
 *   waves, written as one double to workspace[blockIdx] by a plain store.  No atomics, no arrival counter.
 *   The _segments form reads the same positions through the table of fpsg_adam_step_segments (NULL = zeros; the
 *   gradient tensors may start at any 4-byte address): the same thread, the same order, so the same bits as the flat
 *   form on the gathered values.
 * Finalize (one workgroup; one thread does the arithmetic):
 *   S    = workspace[0] + workspace[1] + .. in ascending order from +0.0, fp64
 *   norm = (float)(fabs((double)grad_scale) * sqrt(S))
 *   x    = max_norm / (norm + 1e-6f)            fp32
 *   coef = x if x < 1 or x is NaN, else 1.0f    (torch.clamp(max=1.0) keeps a NaN)
 *   out2[0] = norm;  out2[1] = grad_scale * coef   (one fp32 product: grad_scale itself whenever nothing is clipped)
 *   stats (optional, double[4], updated in place by plain loads and stores -- the stream orders the steps):
 *   [0] += 1; [1] += 1 if coef < 1; [2] += 1 if norm is not finite; [3] = max([3], norm) over the finite norms.
 * fpsg_grad_norm_workspace_bytes(n) = 8 P (0 for n = 0).  Both calls only enqueue (two launches).
 * Errors, all before any launch: FPSG_E_SHAPE for n = 0, nseg < 1, a workspace smaller than
 * fpsg_grad_norm_workspace_bytes(n), max_norm negative or NaN (+inf is accepted and never clips) or a grad_scale that
 * is not finite; FPSG_E_NULL for a null grad, table, workspace or out2; FPSG_E_ALIGN for a grad that is not 16-byte
 * aligned, a workspace, stats or table that is not 8-byte aligned, or a misaligned out2.
 */
size_t fpsg_grad_norm_workspace_bytes(size_t n);
int fpsg_grad_clip_scale(const float* grad, size_t n, float grad_scale, float max_norm, void* workspace,
                         size_t workspace_bytes, float* out2, double* stats, fpsg_stream_t stream);
int fpsg_grad_clip_scale_segments(const float* const* grad_ptrs, const long long* seg_off, int nseg, size_t n,
                                  float grad_scale, float max_norm, void* workspace, size_t workspace_bytes, float* out2,
                                  double* stats, fpsg_stream_t stream);
/* fpsg_adam_step / fpsg_adam_step_segments with the factor on the gradient read from device memory (one float, e.g.
 * out2 + 1 of the calls above; each thread reads it once) instead of passed by value: the same arithmetic, so with
 * *grad_scale_dev == grad_scale the same bits.  The same checks; grad_scale_dev must not be null. */
int fpsg_adam_step_dscale(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                          float beta1, float beta2, float eps, int step, const float* grad_scale_dev,
                          fpsg_stream_t stream);
int fpsg_adam_step_segments_dscale(float* param, const float* const* grad_ptrs, const long long* seg_off, int nseg,
                                   float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                                   float eps, int step, const float* grad_scale_dev, fpsg_stream_t stream);

/* ---- K23: an exponential moving average of the weights inside K7's stream ----------------------------
 * The Adam step of fpsg_adam_step / fpsg_adam_step_segments with a fifth flat buffer of the parameters' layout, the
 * shadow: wherever the step stores a new parameter p it also stores
 *   ema = fma(ema_weight, p - ema, ema)         fp32, one rounding of p - ema and one of the fma
 * with the p it has just computed (never re-read).  ema_weight = 1 - decay_t is the caller's (fpsg_amd/ema.py: the
 * warm-up schedule formed in double, rounded to fp32 once).  5 reads + 4 writes, 36 B per parameter, one launch; a
 * separate pass over parameters and shadow would be a second launch and 12 B.  param, exp_avg and exp_avg_sq get the
 * bits the entry without the shadow gives them.
 * grad_scale_dev may be NULL: the factor on the gradient is then grad_scale, as in fpsg_adam_step.  Otherwise it is
 * read from device memory, as in fpsg_adam_step_dscale (K20), and grad_scale is ignored: one pair of entries serves the
 * plain and the clipped step.  Deterministic: every element is read and written by one thread, no atomics.
 * Errors, all before any launch: those of fpsg_adam_step / fpsg_adam_step_segments; FPSG_E_NULL for a null ema;
 * FPSG_E_ALIGN for an ema that is not 16-byte aligned or a grad_scale_dev that is not 4-byte aligned; FPSG_E_SHAPE for
 * an ema that is param, exp_avg or exp_avg_sq, or an ema_weight that is not a finite number in (0, 1].
 */
int fpsg_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr,
                       float beta1, float beta2, float eps, int step, float grad_scale, const float* grad_scale_dev,
                       float ema_weight, fpsg_stream_t stream);
int fpsg_adam_step_segments_ema(float* param, const float* const* grad_ptrs, const long long* seg_off, int nseg,
                                float* exp_avg, float* exp_avg_sq, float* ema, size_t n, float lr, float beta1,
                                float beta2, float eps, int step, float grad_scale, const float* grad_scale_dev,
                                float ema_weight, fpsg_stream_t stream);
/* a[i] <-> b[i] for i < n, in place: one launch, two reads and two writes per element, no temporary.  It is how a model
 * is evaluated on its averaged weights: the parameters are views of the flat buffer and captured graphs hold their
 * addresses, so the contents move and the pointers do not.  Calling it twice restores every bit.
 * Errors before the launch: FPSG_E_SHAPE for n = 0 or a == b, FPSG_E_NULL, FPSG_E_ALIGN (both 16-byte aligned). */
int fpsg_flat_swap(float* a, float* b, size_t n, fpsg_stream_t stream);

/* ---- K26: area-weighted sampling of a triangle mesh's surface -----------------------------------
 * Makes the point clouds the reference took from pcl_mesh_sampling.  PCL is not pinned; the definition below is the
 * specification.  Two entry points: the mesh's integer CDF, then any number of sample sets from it.
 * verts [V,3] fp32; faces [F,3] int32; cdf [F] uint64; u [m,3] fp32; points [m,3] fp32; face_idx [m] int32.
 * Areas, fp32, every operation rounded on its own (no fused multiply-add), a, b, c the face's vertices:
 *   e1 = b - a, e2 = c - a;  n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x);
 *   area = 0.5 sqrt((nx nx + ny ny) + nz nz), sqrt correctly rounded.
 *   A face with a NaN or infinite area, or with a vertex index outside [0, V), has area 0.
 * Weights: q_f = (uint64) rint((double) area_f / (double) area_max 2^32) (round half to even), 0 for area 0; area_max
 * is the largest area (an integer maximum over the bits: no order of arrival enters).  C_f = q_0 + ... + q_f in
 * uint64: integers, so every scan order gives the same C, and nothing depends on the launch shape.  F <=
 * FPSG_MESH_MAX_FACES keeps C below 2^57.  T = C_{F-1}; T = 0 iff every face has area 0.
 * Samples, one per row of u, each component first clamped to [0, 1 - 2^-24] (NaN -> 0):
 *   t = min((uint64) ((double) u0 (double) T), T - 1)  (the product rounded to double, then truncated);
 *   f = the first face with C_f > t -- a face with q = 0 is never chosen;
 *   s = sqrt(u1); w0 = 1 - s, w1 = s (1 - u2), w2 = s u2;  p = (w0 a + w1 b) + w2 c per coordinate, fp32, no fma.
 * fpsg_mesh_cdf writes cdf; its workspace (fpsg_mesh_cdf_workspace_bytes, 8-byte aligned) holds the areas and block
 * sums; deterministic.  fpsg_mesh_sample takes `total` = cdf[F-1], which the caller reads back from the device:
 * total = 0 is refused with FPSG_E_SHAPE and a message that names the cause, before any launch.  The kernel clamps what
 * it reads from cdf and faces into range, so a foreign cdf gives wrong samples and never an access outside the buffers.
 * Errors, all before any launch: FPSG_E_SHAPE for V, F or m < 1, total = 0 or > F 2^32, a workspace too small;
 * FPSG_E_LIMIT for F > FPSG_MESH_MAX_FACES; FPSG_E_NULL for a null pointer; FPSG_E_ALIGN for a misaligned one (cdf
 * and ws: 8 bytes).  fpsg_mesh_cdf_workspace_bytes returns 0 for a shape the entry refuses.
 */
#define FPSG_MESH_MAX_FACES (1 << 24)
size_t fpsg_mesh_cdf_workspace_bytes(int V, int F);
int fpsg_mesh_cdf(const float* verts, int V, const int32_t* faces, int F, uint64_t* cdf, void* ws, size_t ws_bytes,
                  fpsg_stream_t stream);
int fpsg_mesh_sample(const float* verts, int V, const int32_t* faces, int F, const uint64_t* cdf, uint64_t total,
                     const float* u, int m, float* points, int32_t* face_idx, fpsg_stream_t stream);

/* ---- K27: orthographic Phong views of a triangle mesh -------------------------------------------
 * Makes the view images the reference rendered with Blender (src/preprocess/phong.py, view_generator.py).  The
 * scene file is not pinned; the definition below is the specification.
 * verts [V,3] fp32; faces [F,3] int32; views [n_views,12] fp32: per view the camera's right, up and forward unit
 * vectors and its position c (built by the caller in double, rounded once).  W x H is the SAMPLE resolution, ssaa
 * a divisor of both; the outputs image (uint8) and radiance (fp32) are [n_views, H/ssaa, W/ssaa, 3], face_id (int32,
 * -1 = empty) and depth (fp32, +inf = empty) are [n_views, H, W].  Any output may be NULL, not all.
 * All of the following in fp32 with every operation rounded on its own (no fma), divisions and sqrt correctly rounded.
 * Project, per vertex p and view:  d = p - c;  x = (dx rx + dy ry) + dz rz, y likewise with up, z with forward;
 *   S = max(W, H);  px = (x / ortho_scale) S + W/2;  py = H/2 - (y / ortho_scale) S;
 *   X = (int) rint(clamp(256 px, -2^28, 2^28)), Y likewise.  A vertex whose px, py or z is not finite is invalid, and
 *   so is every face that uses it or an index outside [0, V).
 * Rasterise, per face and view, integers: A2 = (X1-X0)(Y2-Y0) - (Y1-Y0)(X2-X0) in int64; A2 = 0: skipped; A2 < 0:
 *   vertices 1 and 2 swap (both windings are drawn).  For the pixel centre P = (256 i + 128, 256 j + 128):
 *   E0 = edge(1,2), E1 = edge(2,0), E2 = edge(0,1), edge(a,b) = (Xb-Xa)(Py-Ya) - (Yb-Ya)(Px-Xa).  The pixel is covered
 *   iff for every edge E > 0, or E = 0 and the edge is a top or left one: Yb - Ya < 0, or Yb = Ya and Xb - Xa > 0.
 *   Depth: l_k = (float) E_k / (float) A2;  z = (l0 z0 + l1 z1) + l2 z2; a sample with z not finite is dropped.
 *   Z-buffer: per sample the minimum of (key(z) << 32) | face, key = the float's bits mapped to an unsigned integer
 *   of the same order (negative: all bits inverted; otherwise: sign bit set): the nearest face wins, the lowest face
 *   index on equal depth, whatever the order of the launches (64-bit integer atomicMin).
 * Shade, per covered sample, from the face's vertices a, b, c in world space (in the faces' own order): the edges
 *   b - a and c - a, each turned into the camera frame as e = ((wx rx + wy ry) + wz rz, likewise with up, likewise
 *   with forward) -- the camera's distance never enters, so a normal's error depends on the triangle's shape alone;
 *   n = e1 x e2 (components as in K26), len = sqrt((nx nx + ny ny) + nz nz), n = n / len, or (0,0,-1) when
 *   len is 0 or not finite; n = -n when nz > 0 (two-sided).  With the light direction l (unit, camera frame, towards
 *   the light): ndl = (nx lx + ny ly) + nz lz; diff = max(ndl, 0); spec = ndl > 0 ? max(lz - (2 ndl) nz, 0) : 0,
 *   squared log2_shininess times;  colour_c = (ka_c + kd_c diff) + ks_c spec.
 * Resolve, per output pixel: acc = the sum of its covered samples' colours in row-major sample order, k their number,
 *   inv = 1 / ssaa^2, out_c = acc_c inv + bg_c (1 - k inv); bg = the colour params[12..14], or with bg_image (uint8
 *   [H/ssaa, W/ssaa, 3], shared by the views) (float) byte / 255.  radiance = out; image = (uint8) rint(clamp(out,0,1) 255).
 * params (HOST pointer, 15 floats): ka[3], kd[3], ks[3], l[3], bg[3].
 * Workspace: fpsg_mesh_render_workspace_bytes (16-byte aligned): projected vertices, the z-buffer, the list of
 * triangles too large for one thread.
 * Deterministic: the only atomics are the z-buffer's integer minimum and the counter of that list, whose order
 * does not reach any output.  This holds for fpsg_mesh_render_materials and fpsg_mesh_render_smooth too.
 * Errors, all before any launch: FPSG_E_SHAPE for V, F, n_views, W or H < 1, ssaa outside 1..FPSG_RENDER_MAX_SSAA or
 * not a divisor of W and H, an ortho_scale not positive and finite, log2_shininess outside
 * 0..FPSG_RENDER_MAX_LOG2_SHININESS, a workspace too small; FPSG_E_LIMIT for W or H > FPSG_RENDER_MAX_SIZE, n_views >
 * FPSG_RENDER_MAX_VIEWS or F n_views >= 2^31; FPSG_E_NULL for a null verts, faces, views, params or ws, or no output
 * at all; FPSG_E_ALIGN for a misaligned pointer.  fpsg_mesh_render_workspace_bytes returns 0 for a refused shape.
 */
#define FPSG_RENDER_MAX_SIZE 8192
#define FPSG_RENDER_MAX_VIEWS 1024
#define FPSG_RENDER_MAX_SSAA 4
#define FPSG_RENDER_MAX_LOG2_SHININESS 10
size_t fpsg_mesh_render_workspace_bytes(int V, int F, int n_views, int W, int H);
int fpsg_mesh_render(const float* verts, int V, const int32_t* faces, int F, const float* views, int n_views, int W,
                     int H, int ssaa, float ortho_scale, const float* params, int log2_shininess,
                     const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* face_id, float* depth, void* ws,
                     size_t ws_bytes, fpsg_stream_t stream);

/* ---- K28: K27's views with a base colour per face: materials and textures -------------------------
 * For meshes that carry materials (ShapeNet's model_normalized.obj with its .mtl: Kd per part, map_Kd textures).
 * fpsg_mesh_render_materials projects, rasterises and fills the z-buffer with K27's kernels, so face_id and depth are
 * K27's; only the shade pass differs.  Every argument it shares with fpsg_mesh_render means what it means there.
 * All of the following in fp32 with every operation rounded on its own (no fma), divisions correctly rounded.
 * Extra inputs: face_material [F] int32 (device), a value outside [0, M) = no material; face_uv [F,3,2] fp32 (device),
 *   the corners' (u, v) in the face's own vertex order; materials [M,4] fp32 (HOST): Kd r, g, b and the texture index
 *   as an integer value, -1 = none; tex_table [T,3] int32 (HOST): texel offset, width w, height h; texels (device)
 *   uint8 [n_texels, 3], RGB, every texture row-major from its TOP row, all textures back to back.
 *   params (HOST pointer, 17 floats): K27's 15, then ambient and diffuse.
 *   M = 0: face_material and materials may be NULL.  T = 0: face_uv, tex_table and texels may be NULL.
 * Shade, per covered sample of face f: diff and spec are K27's.
 *   No material: colour_c = (ka_c + kd_c diff) + ks_c spec -- K27's colour, so a call in which no face has a material
 *   gives fpsg_mesh_render's image, radiance, face_id and depth bit for bit.
 *   Material with base colour b:  a_c = ambient b_c;  d_c = diffuse b_c;  colour_c = (a_c + d_c diff) + ks_c spec.
 * Base colour: b = Kd when the material has no texture, or when any of the face's six uv numbers is not finite.
 *   Otherwise b is the texel colour alone (Kd is not multiplied in: many materials carry a black Kd beside a map_Kd).
 * uv at the sample: from the snapped vertices of the face's corners 0, 1, 2 and the sample's centre P, as K27
 *   rasterises: A2 in int64; A2 < 0: corners 1 and 2 swap, and their uv with them, A2 = -A2.  E0 = edge(1,2),
 *   E1 = edge(2,0), E2 = edge(0,1) in int64;  l_k = (float) E_k / (float) A2;
 *   u = (l0 u0 + l1 u1) + l2 u2;  v = (l0 v0 + l1 v1) + l2 v2.  (Orthographic: affine interpolation is the correct one.)
 * Lookup in the texture (w, h), which repeats: tu = u - floor(u), and tu = 0 unless 0 <= tu < 1 (a tu rounded up to
 *   1, a NaN from an overflow); tv likewise.  x = tu w - 0.5;  y = (1 - tv) h - 0.5 (v = 0 is the bottom row, as in OBJ).
 *   x0 = floor(x), fx = x - x0, gx = 1 - fx; y0, fy, gy likewise.  The four neighbours are the texels
 *   (x0 mod w, y0 mod h), (x0+1 mod w, y0 mod h), (x0 mod w, y0+1 mod h), (x0+1 mod w, y0+1 mod h) with values
 *   c00, c10, c01, c11, each channel (float) byte / 255, and weights w00 = gx gy, w10 = fx gy, w01 = gx fy, w11 = fx fy:
 *   b_c = ((w00 c00 + w10 c10) + w01 c01) + w11 c11.
 *   Wrapped neighbours make b a continuous function of (u, v), also across the texture's seam: a last-bit difference
 *   in u moves b by a last bit's worth and never to the texture's far side.  No mipmaps, no gamma: bytes are values.
 * Resolve and outputs: K27's.
 * Workspace: fpsg_mesh_render_materials_workspace_bytes (16-byte aligned): K27's, then the two host tables, which the
 * entry copies there with hipMemcpyAsync on the stream: pageable arrays (malloc, numpy) are read before it returns,
 * pinned ones must stay unchanged until the stream has passed the call.
 * Errors, all before any launch or copy: those of fpsg_mesh_render; FPSG_E_SHAPE for a negative M, T or n_texels, a
 * texture index that is not an integer in [-1, T), a tex_table entry with offset < 0, w < 1, h < 1 or
 * offset + w h > n_texels; FPSG_E_LIMIT for M > FPSG_RENDER_MAX_MATERIALS, T > FPSG_RENDER_MAX_TEXTURES or n_texels >
 * FPSG_RENDER_MAX_TEXELS; FPSG_E_NULL for a null face_material or materials with M > 0, a null face_uv, tex_table
 * or texels with T > 0; FPSG_E_ALIGN for a misaligned pointer.  The workspace function returns 0 for a refused shape.
 */
#define FPSG_RENDER_MAX_MATERIALS 65536
#define FPSG_RENDER_MAX_TEXTURES 4096
#define FPSG_RENDER_MAX_TEXELS (1 << 28)
size_t fpsg_mesh_render_materials_workspace_bytes(int V, int F, int n_views, int W, int H, int M, int T);
int fpsg_mesh_render_materials(const float* verts, int V, const int32_t* faces, int F, const int32_t* face_material,
                               const float* face_uv, const float* materials, int M, const int32_t* tex_table, int T,
                               const uint8_t* texels, long long n_texels, const float* views, int n_views, int W, int H,
                               int ssaa, float ortho_scale, const float* params, int log2_shininess,
                               const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* face_id, float* depth,
                               void* ws, size_t ws_bytes, fpsg_stream_t stream);

/* ---- K29: orthographic Phong views of point clouds, every point a small sphere ---------------------
 * Shows what the model generates with the cameras of the views it was conditioned on: B clouds in one call, each seen
 * by all the views, with occlusion, shading and an optional colour per point.  Every argument it shares with
 * fpsg_mesh_render means what it means there.
 * points [B,N,3] fp32; colors [B,N,3] uint8 or NULL; views [n_views,12] as K27; W x H the SAMPLE resolution, ssaa (1, 2
 * or 4) a divisor of both; ortho_scale and radius in world units; params (HOST pointer, 17 floats) in K28's layout:
 * ka[3], kd[3], ks[3], l[3], bg[3], ambient, diffuse; bg_image optional, as K27, shared by the clouds and the views.
 * Outputs, any may be NULL, not all: image (uint8) and radiance (fp32) [B, n_views, H/ssaa, W/ssaa, 3]; point_id (int32,
 * -1 = empty) and depth (fp32, +inf = empty) [B, n_views, H, W].
 * All of the following in fp32 with every operation rounded on its own (no fma), divisions and sqrt correctly rounded.
 * Project, per point, view and cloud: K27's vertex projection, which gives the snapped integers X, Y and the depth z.  A
 *   point whose px, py or z is not finite is invalid and draws nothing.
 * Radius in snapped units, by the entry on the host in double:
 *   R = llrint(256 (radius / ortho_scale) max(W, H));  R < 1 or R > 256 FPSG_POINTS_MAX_RADIUS_PX is refused.
 * Cover, at the sample centre P = (256 i + 128, 256 j + 128): dx = Px - X; dy = Py - Y; q = dx dx + dy dy in int64.  The
 *   sample is covered iff q < R R: strict and in integers, so there is no rounding and no tie rule.
 * Depth of the sphere at the sample: t = (float) q / (float) (R R);  c = sqrt(1 - t);  z_s = z - radius c.  (When t
 *   rounds to 1, c is 0.)  A sample with z_s not finite is dropped.
 * Z-buffer: per sample the minimum of (key(z_s) << 32) | point index, key as K27: the nearest sphere wins, the lowest
 *   point index on equal depth, whatever the order of the launches.
 * Shade, per covered sample, from the winner's X, Y and the sample centre: the normal in the camera frame is
 *   nx = (float) dx / (float) R;  ny = -((float) dy / (float) R);  nz = -c, not renormalised.  ndl, diff, spec and the
 *   squaring as K27 with that n.  Without colors: colour_c = (ka_c + kd_c diff) + ks_c spec.  With colors: the base
 *   colour is b_c = (float) byte_c / 255, and a_c = ambient b_c;  d_c = diffuse b_c;  colour_c = (a_c + d_c diff) +
 *   ks_c spec, as K28 forms it from a base colour.
 * Resolve and image: K27's, per cloud and view.
 * Workspace: fpsg_points_render_workspace_bytes = 16 B n_views N bytes (16-byte aligned): one record per (cloud, view,
 * point).  There is no z-buffer in memory.  Deterministic (integer LDS atomics only).
 * Errors, all before any launch or copy: FPSG_E_SHAPE for B, N, n_views, W or H < 1, ssaa not 1, 2 or 4 or not a divisor
 * of W and H, an ortho_scale or radius not positive and finite, R out of range, log2_shininess outside
 * 0..FPSG_RENDER_MAX_LOG2_SHININESS, a workspace too small; FPSG_E_LIMIT for N > FPSG_POINTS_MAX_N, W or H >
 * FPSG_RENDER_MAX_SIZE, n_views > FPSG_RENDER_MAX_VIEWS or B n_views >= 65536; FPSG_E_NULL for a null points, views,
 * params or ws, or no output at all; FPSG_E_ALIGN for a misaligned pointer.  fpsg_points_render_workspace_bytes returns
 * 0 for a refused shape.
 */
#define FPSG_POINTS_MAX_N 16384
#define FPSG_POINTS_MAX_RADIUS_PX 64
size_t fpsg_points_render_workspace_bytes(int B, int N, int n_views, int W, int H);
int fpsg_points_render(const float* points, const uint8_t* colors, int B, int N, const float* views, int n_views, int W,
                       int H, int ssaa, float ortho_scale, float radius, const float* params, int log2_shininess,
                       const uint8_t* bg_image, uint8_t* image, float* radiance, int32_t* point_id, float* depth,
                       void* ws, size_t ws_bytes, fpsg_stream_t stream);

/* ---- K30: the uint8 views of an episode -> the float32 batch the image encoder reads ----------------
 * One launch selects, resamples, colour-jitters and normalises the images of an episode.  All pointers are device
 * memory.
 * src [n_src,Hs,Ws,3] uint8, HWC as PIL gives it; sel [n] int32: the source image of output image k, entries may repeat
 * and come in any order; geom [n,4] int32 = (x0, y0, step, 0) in 1/256 source pixel, or NULL for the identity
 * (0, 0, 256); color [n,4] fp32 = (brightness, contrast, saturation, 0), or NULL for no photometric step;
 * out [n,3,Ho,Wo] fp32.
 * Sample position.  For output pixel (i, j), column i < Wo and row j < Ho:
 *   X = x0 + i*step, Y = y0 + j*step, as int32.  The entry refuses shapes and the wrapper values where these could
 *   overflow: |x0|, |y0| <= 2^24, 1 <= step <= 2^16, Ho, Wo <= 8192; the kernel clamps x0, y0 and step to those ranges.
 *   ix = X >> 8 (arithmetic shift, a floor), fx = X & 255.  The same for y.
 *   The taps ix, ix+1, iy, iy+1 are clamped to the image (clamp to edge): ix0 = min(max(ix, 0), Ws-1),
 *   ix1 = min(max(ix+1, 0), Ws-1), and so for the rows.
 * Blend.  Integer bilinear blend per channel, p the uint8 pixel:
 *   a_r = p[r][ix0]*(256-fx) + p[r][ix1]*fx for the two rows r.
 *   v = a_0*(256-fy) + a_1*fy.
 *   v is an integer in [0, 255*65536], below 2^24, so (float)v is exact.
 *   x = (float)v / 16711680.0f, a correctly rounded division.
 *   At fx = fy = 0 this equals p / 255.0f bit for bit.
 * Photometric step, only when color is not NULL.  It is applied always then, also at (0,1,1), in fp32 and in this order,
 * every operation rounded on its own (no fma), br = brightness, c = contrast, s = saturation:
 *   l = (0.299f*r + 0.587f*g) + 0.114f*b.
 *   Per channel t = l + s*(x - l).
 *   u = (t - 0.5f)*c + (0.5f + br).
 *   u = min(max(u, 0), 1).
 * Output.  y = (x_or_u - 0.5f) / 0.5f.
 * Bad sel entry.  An entry outside [0, n_src) yields an image of quiet NaNs; src is not read for it.
 * Errors, all before any HIP call: FPSG_E_SHAPE for n_src, Hs, Ws, n, Ho or Wo < 1; FPSG_E_LIMIT for Hs, Ws, Ho or Wo >
 * FPSG_VIEWS_MAX_SIZE or n > FPSG_VIEWS_MAX_IMAGES; FPSG_E_NULL for a null src, sel or out; FPSG_E_ALIGN for a sel,
 * geom, color or out that is not 4-byte aligned.  geom is device memory: the range of x0, y0 and step is checked by the
 * Python wrapper on the host copy before the upload, and clamped in the kernel.
 */
#define FPSG_VIEWS_MAX_SIZE 8192
#define FPSG_VIEWS_MAX_IMAGES 65535
#define FPSG_VIEWS_MAX_OFFSET (1 << 24)
#define FPSG_VIEWS_MAX_STEP (1 << 16)
int fpsg_episode_views(const uint8_t* src, int n_src, int Hs, int Ws, const int32_t* sel, int n, const int32_t* geom,
                       const float* color, float* out, int Ho, int Wo, fpsg_stream_t stream);

/* ---- K31a: area-weighted vertex normals of meshes that share their faces ---------------------------
 * For the meshes a decoder generates: B vertex arrays on one topology (the patches' regular grids), so the faces and
 * the table below are built once and serve every mesh.  All pointers are device memory.
 * verts [B,V,3] fp32; faces [F,3] int32; normals [B,V,3] fp32 (output).
 * Corner table, built by the caller once per topology: offsets [V+1] int32 and corner_faces [n] int32.  The slice
 *   corner_faces[offsets[v] .. offsets[v+1]) lists, in ascending order, the faces that name vertex v, once per corner
 *   that names it (a face (v, v, w) appears twice in v's slice).  A face with an index outside [0, V) is listed
 *   nowhere, so n <= 3 F.
 * All of the following in fp32 with every operation rounded on its own (no fma), division and sqrt correctly rounded.
 * Per mesh and vertex v:  s = (0, 0, 0);  for every entry f of v's slice, in order, with the face's vertices a, b, c in
 *   the faces' own order:  e1 = b - a;  e2 = c - a;
 *   nx = e1y e2z - e1z e2y;  ny = e1z e2x - e1x e2z;  nz = e1x e2y - e1y e2x  (components as in K26, NOT normalised:
 *   the face's normal times twice its area, which is the area weighting);  s = s + n, per component.
 *   len = sqrt((sx sx + sy sy) + sz sz);  normal = s / len per component, or (0, 0, 0) when len is 0 or not finite.
 * What the kernel does with a table that does not follow the rule: a slice is clamped to 0 <= begin <= end <= n, an
 *   entry outside [0, F) is skipped, and so is a face with an index outside [0, V).  Such a table gives other normals
 *   than the definition's, and never a read or write outside the arrays.
 * Gather form: one thread per (mesh, vertex), no atomics; bitwise the same on every run.
 * Errors, all before the launch: FPSG_E_SHAPE for B, V or F < 1, n < 0 or n > 3 F; FPSG_E_LIMIT for
 * B > FPSG_NORMALS_MAX_MESHES, V or F > FPSG_MESH_MAX_FACES; FPSG_E_NULL for a null verts, faces, offsets or normals,
 * or a null corner_faces with n > 0; FPSG_E_ALIGN for a misaligned pointer.
 */
#define FPSG_NORMALS_MAX_MESHES 65535
int fpsg_mesh_vertex_normals(const float* verts, int B, int V, const int32_t* faces, int F, const int32_t* offsets,
                             const int32_t* corner_faces, int n, float* normals, fpsg_stream_t stream);

/* ---- K31b: K28's views lit by interpolated corner normals (smooth shading) --------------------------
 * fpsg_mesh_render_smooth projects, rasterises and fills the z-buffer with K27's kernels, so face_id and depth are
 * K27's; the base colour, the resolve and the outputs are K28's; only the normal that the light's terms use differs.
 * Every argument it shares with fpsg_mesh_render_materials means what it means there (params: 17 floats; M = 0 and
 * T = 0 as there: without materials the colours are K27's ka, kd).
 * Extra input: face_normals [F,3,3] fp32 (device): per face the normals of its corners 0, 1, 2 in world space, in the
 *   layout of face_uv.  They need not have unit length.
 * All of the following in fp32 with every operation rounded on its own (no fma), divisions and sqrt correctly rounded.
 * Shade, per covered sample of face f:
 *   g = K27's unit face normal in the camera frame, after its fallback (0,0,-1) and its two-sided flip (g_z <= 0).
 *   l0, l1, l2 = K28's barycentrics of the sample centre from the snapped corners: A2 in int64; A2 < 0: corners 1 and
 *     2 swap, and their normals n1 and n2 with them; E0 = edge(1,2), E1 = edge(2,0), E2 = edge(0,1);
 *     l_k = (float) E_k / (float) A2.
 *   m = (l0 n0 + l1 n1) + l2 n2, per component (world space).
 *   t = ((mx rx + my ry) + mz rz, likewise with up, likewise with forward): m in the camera frame, as K27 turns edges.
 *   len = sqrt((tx tx + ty ty) + tz tz).
 *   len is 0 or not finite (zero normals, NaN, inf, opposed corners):  c = g.
 *   Otherwise c = t / len per component;  side = (cx gx + cy gy) + cz gz;  c = -c when side < 0: the interpolated
 *     normal follows the side of the face that the camera sees, as g does.
 *   ndl = (cx lx + cy ly) + cz lz;  diff = max(ndl, 0);  spec = ndl > 0 ? max(lz - (2 ndl) cz, 0) : 0, squared
 *     log2_shininess times;  colour: K28's from diff, spec and the face's base colour.
 *   Corner normals that are all zero, or all NaN, therefore give fpsg_mesh_render_materials' outputs bit for bit.
 * Workspace: fpsg_mesh_render_smooth_workspace_bytes = fpsg_mesh_render_materials_workspace_bytes.
 * Errors, all before any launch or copy: those of fpsg_mesh_render_materials; FPSG_E_NULL for a null face_normals,
 * FPSG_E_ALIGN for a misaligned one.
 */
size_t fpsg_mesh_render_smooth_workspace_bytes(int V, int F, int n_views, int W, int H, int M, int T);
int fpsg_mesh_render_smooth(const float* verts, int V, const int32_t* faces, int F, const int32_t* face_material,
                            const float* face_uv, const float* face_normals, const float* materials, int M,
                            const int32_t* tex_table, int T, const uint8_t* texels, long long n_texels,
                            const float* views, int n_views, int W, int H, int ssaa, float ortho_scale,
                            const float* params, int log2_shininess, const uint8_t* bg_image, uint8_t* image,
                            float* radiance, int32_t* face_id, float* depth, void* ws, size_t ws_bytes,
                            fpsg_stream_t stream);

/* ---- K32: the nearest triangle of every point (point-to-mesh distance) ------------------------------
 * For every point of B clouds the nearest point of a triangle mesh, by brute force over the faces.  The definition is
 * the project's own (parity with published code: UNPINNED).  All pointers are device memory.
 * points [B,N,3] fp32; verts [V,3] fp32 shared by the B clouds (verts_per_mesh = 0) or [B,V,3] (verts_per_mesh = 1);
 * faces [F,3] int32, shared.  Outputs: dist2 [B,N] fp32, face [B,N] int32, closest [B,N,3] fp32 or NULL, bary [B,N,3]
 * fp32 or NULL.
 * All of the following in fp32 with every operation rounded on its own (no fma), the division correctly rounded.
 *   dot(x, y) = (x0 y0 + x1 y1) + x2 y2;   rc(x) = 1.0f / x when x > 0 and x is finite, else 0;
 *   clamp(t) = min(max(t, 0), 1) and least(x, y, ..) with the minimum and maximum that return the other operand when one
 *   is NaN (fminf, fmaxf).  Vector operations are per component.
 * Per face with corners a, b, c (indices in [0, V); a face with an index outside is skipped):
 *   e0 = b - a;  e1 = c - a;  e2 = c - b;
 *   d00 = dot(e0,e0);  d01 = dot(e0,e1);  d11 = dot(e1,e1);  d22 = dot(e2,e2);  det = d00 d11 - d01 d01;
 *   r0 = rc(d00);  r1 = rc(d11);  r2 = rc(d22);  rd = rc(det).
 * Per point p and face, four candidates, each a point of the triangle:
 *   ap = p - a;  bp = p - b;  s0 = dot(ap,e0);  s1 = dot(ap,e1);  s2 = dot(bp,e2);
 *   t0 = clamp(s0 r0);  q0 = a + e0 t0;     t1 = clamp(s1 r1);  q1 = a + e1 t1;     t2 = clamp(s2 r2);  q2 = b + e2 t2;
 *   v = (d11 s0 - d01 s1) rd;  w = (d00 s1 - d01 s0) rd;  qI = a + (e0 v + e1 w),
 *     valid only when rd > 0 and v >= 0 and w >= 0 and v + w <= 1;
 *   d(q) = dot(p - q, p - q);   the pair's value m = least(d(q0), d(q1), d(q2), and d(qI) when valid); its candidate is
 *   the first of q0, q1, q2, qI whose d equals m.  A candidate whose d is NaN never wins.
 *   A sliver or a face without area (rd = 0, or v, w spoilt by cancellation) therefore degrades to the nearest point of
 *   its edges, and a face collapsed to one point (r0 = r1 = r2 = 0, every t = 0) to the distance to that point.
 * Per point: best = +inf, face = -1; for the faces in ascending order: m < best: best = m, face = f.  The minimum is exact,
 *   so the lowest face id wins ties and the bits depend neither on the tiling nor on chunks.
 *   dist2 = best;  closest = the winning pair's candidate q;  bary = its weights on (a, b, c):
 *   q0: (1 - t0, t0, 0);  q1: (1 - t1, 0, t1);  q2: (0, 1 - t2, t2);  qI: ((1 - v) - w, v, w).
 *   A point with a non-finite coordinate, or a mesh without a usable face, keeps dist2 = +inf and face = -1; its closest
 *   and bary are NaN.
 * The faces are split over `chunks` slices of ceil(F / chunks) consecutive faces (1..FPSG_POINT_MESH_MAX_CHUNKS; <= 0:
 * the library chooses from B, N and F); every slice writes a packed 64-bit (dist2 bits << 32 | face) partial per point
 * to the workspace (non-negative floats order as unsigned integers) and a second kernel takes their minimum in
 * ascending order and recomputes closest and bary for the winner with the same operations.  No atomics: bitwise the
 * same on every run.  The kernels never read outside the arrays, whatever faces holds.
 * Workspace: fpsg_point_mesh_workspace_bytes(B, N, F, chunks) bytes, 8-byte aligned; 0 for a shape the entry refuses.
 * Errors, all before any launch, shape and limit checks in front of the pointer checks: FPSG_E_SHAPE for B, N, V or
 * F < 1, verts_per_mesh not 0 or 1 or a workspace too small; FPSG_E_LIMIT for N > FPSG_POINT_MESH_MAX_POINTS, B >
 * FPSG_POINT_MESH_MAX_MESHES, B N > FPSG_POINT_MESH_MAX_TOTAL, V or F > FPSG_MESH_MAX_FACES or chunks >
 * FPSG_POINT_MESH_MAX_CHUNKS; FPSG_E_NULL for a null points, verts, faces, dist2, face or ws; FPSG_E_ALIGN for a
 * misaligned pointer (ws: 8 bytes).
 */
#define FPSG_POINT_MESH_MAX_POINTS (1 << 20)
#define FPSG_POINT_MESH_MAX_MESHES 65535
#define FPSG_POINT_MESH_MAX_TOTAL (1 << 26)
#define FPSG_POINT_MESH_MAX_CHUNKS 64
size_t fpsg_point_mesh_workspace_bytes(int B, int N, int F, int chunks);
int fpsg_point_mesh_distance(const float* points, int B, int N, const float* verts, int V, int verts_per_mesh,
                             const int32_t* faces, int F, int chunks, float* dist2, int32_t* face, float* closest,
                             float* bary, void* ws, size_t ws_bytes, fpsg_stream_t stream);

/* ---- K33: normals of a point cloud (k-NN PCA, sign rules, orientation along a spanning forest) ------------
 * The pipeline of Hoppe et al. (1992), as PCL and Open3D run it: the k nearest neighbours of every point, PCA of the
 * neighbourhood, the eigenvector of the smallest eigenvalue; then one sign per point.  The published codes are not
 * pinned; the definition below is the specification (parity UNPINNED).  All pointers are device memory.
 *
 * K33a, fpsg_point_normals.  Inputs: B clouds xyz [N,3] fp32, FPSG_NORMALS_POINTS_MIN_K <= k <= FPSG_NORMALS_POINTS_MAX_K,
 * N >= k + 1; ref [B,3] fp32 (sign_mode 1 and 2; may be NULL with sign_mode 0).  Outputs: normals [B,N,3] fp32; variation
 * [B,N] fp32 or NULL; nbr_idx [B,N,k] int32 or NULL.
 *   d2(i,j)  = fma(dz,dz, fma(dy,dy, dx*dx)), dx = x_j - x_i                              (K1's sq_dist, as K21)
 *   K(i)     = the k indices j != i with the smallest (d2(i,j), j) in lexicographic order (ties: the lower index),
 *              stored nearest first.  j == i is skipped by index: a duplicate of point i is a neighbour at distance 0.
 *              The set is exact and bitwise the same on every run.  A slot that no candidate entered (non-finite
 *              coordinates only) holds i itself, so every stored index is in [0, N).
 *   The neighbourhood is {i} and K(i): k + 1 points.  All of the following in fp32, every operation rounded on its own:
 *   o_s      = x_j - x_i per component for the s-th neighbour j (the point's own offset is 0; the differences are exact
 *              where the cloud lies far from the origin)
 *   mu       = (o_1 + o_2 + .. + o_k) / (k + 1), summed from +0 in list order
 *   C        = mu mu^T + sum_s (o_s - mu)(o_s - mu)^T, in list order: centred BEFORE the products, six entries
 *   trace    = (C00 + C11) + C22.  Where trace is 0, not finite, or so small that 1 / trace is not finite:
 *              normal = (0,0,0), variation = 0.
 *   A        = C * (1 / trace); eight cyclic Jacobi sweeps over the planes (0,1), (0,2), (1,2) (a fixed count) with
 *              theta = (a_qq - a_pp) / (2 a_pq), t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)), t = 0 where a_pq == 0,
 *              c = 1 / sqrt(t^2 + 1), s = t c; the eigenvalues are the diagonal left over, lambda0 the smallest (the
 *              lowest position on ties), the normal its column of the accumulated rotations times 1 / sqrt of its
 *              squared length.
 *   variation = min(max(lambda0, 0) / ((a00 + a11) + a22), 1/3): Pauly's surface variation, in [0, 1/3].
 *   sign_mode 0 (canonical): the component of largest magnitude is positive, the lowest axis wins ties; the output is
 *              a function of the cloud alone.
 *   sign_mode 1 (toward ref[b]): with e = (nx (rx - px) + ny (ry - py)) + nz (rz - pz) on the canonical normal, the
 *              normal is negated where e < 0.   sign_mode 2 (away from ref[b]): negated where e > 0.
 *              Where e is exactly 0 (or NaN) the canonical sign stays.
 * Two launches (the sweep; one thread per point for the PCA); the lists pass through nbr_idx, or through the workspace
 * (fpsg_point_normals_workspace_bytes) when nbr_idx is NULL.
 *
 * K33b, fpsg_point_normals_orient.  Inputs: xyz, normals_in [B,N,3] fp32, nbr_idx [B,N,k] int32 (K33a's, or any table),
 * axis in 0..2.  Outputs: normals_out [B,N,3] fp32 (must not overlap normals_in), parent [B,N] int32 or NULL.
 *   edges    : i ~ j iff j is an entry of row i or i is an entry of row j; an entry outside [0, N), or equal to its own
 *              row, is no edge.
 *   w(i,j)   = 1 - |(nx mx + ny my) + nz mz| on normals_in, fp32, every operation rounded on its own: bitwise
 *              symmetric and independent of any sign.  A zero normal is an ordinary vertex of weight 1 to everyone.
 *   forest   : Prim's with K24's tie rules.  Every non-tree vertex keeps a key and a parent, replaced only by a
 *              STRICTLY smaller weight to a vertex that joins; each step adds the non-tree vertex with the smallest
 *              (key, index).  When no non-tree vertex has a key, the next root is the non-tree vertex with the largest
 *              xyz[., axis], the lowest index on ties; the first root is chosen the same way.  Exactly N steps.
 *   signs    : a root is negated where its `axis` component is < 0; a vertex v that joins under parent u is negated
 *              where (ux vx + uy vy) + uz vz < 0 with u's ORIENTED normal.  parent is -1 at roots.
 * One workgroup per cloud; keys and parents live in LDS (8 N bytes: N <= FPSG_NORMALS_POINTS_MAX_N fits the 160 KB).  The
 * reverse lists come from two gather sweeps (count, fill) into the workspace: three launches.
 *
 * Both: no atomics, nothing passes between workgroups inside a launch; a cloud's results depend neither on B nor on its
 * place in the batch and are bitwise the same on every run; non-finite coordinates or normals give unspecified values
 * for that cloud only; no index outside [0, N) is ever stored or dereferenced; the calls only enqueue work on `stream`.
 * Errors, all before any launch, shape and limit checks in front of the pointer checks: FPSG_E_SHAPE for B < 1, k
 * outside 3..32, N < k + 1, sign_mode or axis outside 0..2, a workspace too small; FPSG_E_LIMIT for N >
 * FPSG_NORMALS_POINTS_MAX_N or B > FPSG_NORMALS_POINTS_MAX_B; FPSG_E_NULL for a null xyz, normals, normals_in, nbr_idx (K33b),
 * normals_out or ws, or a null ref with sign_mode 1 or 2; FPSG_E_ALIGN for a misaligned pointer.  The workspace functions
 * return 0 for a shape the entries refuse.
 */
#define FPSG_NORMALS_POINTS_MIN_K 3
#define FPSG_NORMALS_POINTS_MAX_K 32
#define FPSG_NORMALS_POINTS_MAX_N 16384
#define FPSG_NORMALS_POINTS_MAX_B 65535
size_t fpsg_point_normals_workspace_bytes(int B, int N, int k);
int fpsg_point_normals(const float* xyz, int B, int N, int k, int sign_mode, const float* ref, float* normals,
                       float* variation, int32_t* nbr_idx, void* ws, size_t ws_bytes, fpsg_stream_t stream);
size_t fpsg_point_normals_orient_workspace_bytes(int B, int N, int k);
int fpsg_point_normals_orient(const float* xyz, const float* normals_in, const int32_t* nbr_idx, int B, int N, int k,
                              int axis, float* normals_out, int32_t* parent, void* ws, size_t ws_bytes,
                              fpsg_stream_t stream);

/* ---- K34: surface reconstruction from an oriented cloud (implicit field, marching-tetrahedra isosurface) -----------
 * One closed, consistently oriented triangle mesh from a cloud with normals (K33's, or any): an implicit-moving-least-
 * squares field of signed tangent-plane distances on a regular grid (Kolluri 2005; Shen et al. 2004) with a compactly
 * supported polynomial weight, and the zero level set of that field by marching tetrahedra on the Kuhn split of the
 * cells.  The definition below is the specification (parity UNPINNED).  All pointers are device memory.
 * All arithmetic in fp32 with every operation rounded on its own (no fma), divisions correctly rounded; max(x, 0)
 * returns 0 when x is NaN (fmaxf).
 *
 * K34a, fpsg_implicit_field.  Inputs: points, normals [B,N,3] fp32; origin [B,3], cell [B], radius [B] fp32 (device
 * memory: no host read); G nodes per side.  Outputs: field [B,G,G,G] fp32; weight [B,G,G,G] fp32 or NULL.
 *   Node (i,j,k) of cloud b is field[b][i][j][k] and lies at x = origin + (float)i * cell per axis (the multiply, then
 *   the add).  inv = 1 / (radius * radius), once per cloud.  From num = den = +0, over the points j in ascending order:
 *     d  = x - p_j per component;   d2 = (dx*dx + dy*dy) + dz*dz;   t = max(1 - d2*inv, 0);   w = (t*t)*t;
 *     s  = (dx*nx + dy*ny) + dz*nz;   num = num + w*s;   den = den + w.
 *   A point with a non-finite coordinate or normal component contributes nothing.
 *   field = den > 0 ? num / den : NaN (the quiet NaN 0x7fc00000);   weight = den.
 *   The weight is a polynomial of the squared distance: no exp, no sqrt, and a point outside a node's ball contributes
 *   exactly +0, so the kernel skips the points whose ball cannot reach a brick of FPSG_FIELD_BRICK^3 nodes (a test
 *   that is conservative in floating point; iso_surface.h derives its margin) without changing a bit.  This holds for
 *   a radius whose square and its reciprocal are normal fp32 numbers and for products w*s that do not overflow;
 *   outside that the values are unspecified (never an access outside the arrays).  The cloud passes through LDS in
 *   tiles of FPSG_FIELD_TILE points.  One launch; no atomics, nothing passes between workgroups.
 *
 * K34b, fpsg_iso_classify and fpsg_iso_emit.  Input: field [B,G,G,G] (K34a's, or any).
 *   A node is inside when field < 0; 0, -0 and NaN are not inside.  Every cell (its lowest corner (i,j,k), i,j,k < G-1)
 *   is split into six tetrahedra: for the permutations (a,b,c) of the axes (0 = i, 1 = j, 2 = k) in lexicographic order
 *   012, 021, 102, 120, 201, 210, the corners in path order 000, +e_a, +e_a+e_b, 111.  The split is the same in every
 *   cell, so neighbouring cells agree on every face diagonal.
 *   A grid edge belongs to its lower node and has one of 7 classes, the step (di,dj,dk) in the order 100, 010, 001, 110,
 *   101, 011, 111.  It is active when both ends are finite and exactly one is inside; flags = the bit set of a node's
 *   active owned classes.  An active edge carries one vertex: t = f0 / (f0 - f1) from the owner toward the far node, the
 *   coordinate x0 + t * cell on the axes the class steps along and x0 on the others (x0 the owner's node position).
 *   A tetrahedron emits triangles only when its four corners are finite.  With the path corners numbered 0..3, inside
 *   ones i < j < .. and outside ones k < l < ..: one inside: the triangle (i,k),(i,l),(i,m) on its three edges; three
 *   inside: (i,k),(j,k),(m,k) on the outside corner's edges; two inside: the quad (i,k),(i,l),(j,l),(j,k) as
 *   [(i,k),(i,l),(j,l)] and [(i,k),(j,l),(j,k)].  Where the normal of a triangle so listed (corners at their unit-cube
 *   positions, vertices at the edge midpoints) does not look from the inside corners' centroid toward the outside
 *   corners', the last two vertices of each triangle of the case are exchanged: the mesh is counter-clockwise seen
 *   from outside, its normals look toward positive field.  The 6 x 16 table is generated from this rule at compile time.
 *   fpsg_iso_classify writes node_edges [B,G^3] int32 (popcount(flags), 0..7) and cell_tris [B,G^3] int32 (the triangles
 *   of the cell whose lowest corner is the node, 0..12; 0 where i, j or k is G-1).  The caller turns both into exclusive
 *   64-bit offsets over all B G^3 nodes (edge_offset, tri_offset) and sizes the outputs by the totals n_verts, n_faces.
 *   fpsg_iso_emit recomputes the flags from the field and writes, packed over the clouds, verts [n_verts,3] fp32 in
 *   ascending node order, then class order, and faces [n_faces,3] int32 in ascending cell, tetrahedron, then table
 *   order; an edge's vertex id is edge_offset[owner] + popcount(flags[owner] & ((1 << class) - 1)) minus the cloud's
 *   own first offset, so indices are local to their cloud.  vert_range, face_range [B+1] int64 (or NULL): cloud b owns
 *   verts[vert_range[b] : vert_range[b+1]] and faces[face_range[b] : face_range[b+1]].  Offsets that lie give a wrong
 *   mesh, never a write outside [0, n_verts) x [0, n_faces).  verts or faces may be NULL when its count is 0.
 *   One thread per node in both kernels; no atomics; bitwise the same on every run.
 *
 * Errors, all on the host before any HIP call, in this order: FPSG_E_SHAPE for B or N < 1, G < FPSG_ISO_MIN_GRID, a
 * negative n_verts or n_faces; FPSG_E_LIMIT for G > FPSG_ISO_MAX_GRID, B G^3 >
 * FPSG_ISO_MAX_NODES or N > FPSG_NORMALS_POINTS_MAX_N; FPSG_E_NULL for a null pointer other than weight, vert_range,
 * face_range (and verts, faces with a zero count); FPSG_E_ALIGN for a misaligned pointer (the int64 arrays: 8 bytes).
 */
#define FPSG_ISO_MIN_GRID 2
#define FPSG_ISO_MAX_GRID 256
#define FPSG_ISO_MAX_NODES (1 << 28)
#define FPSG_FIELD_BRICK 8
#define FPSG_FIELD_TILE 256
int fpsg_implicit_field(const float* points, const float* normals, int B, int N, const float* origin, const float* cell,
                        const float* radius, int G, float* field, float* weight, fpsg_stream_t stream);
int fpsg_iso_classify(const float* field, int B, int G, int32_t* node_edges, int32_t* cell_tris, fpsg_stream_t stream);
int fpsg_iso_emit(const float* field, const float* origin, const float* cell, int B, int G, const int64_t* edge_offset,
                  const int64_t* tri_offset, long long n_verts, long long n_faces, float* verts, int32_t* faces,
                  int64_t* vert_range, int64_t* face_range, fpsg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FPSG_HIP_H */
