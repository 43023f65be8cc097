/*
 * beast_hip.h -- C-ABI of libbeast_hip.so, the MI355X (gfx950) hot path of BEAST.
 *
 * The reference (Dont4rootMe/beast_tokenizer) has no native boundary: its
 * "plugin point" is the mp_pytorch UniformBSpline object, beast/utils.py and the
 * HF `tokenizers` BpeTrainer.  Each entry point below replaces one of those call
 * sites (cited per function) and is what a ctypes / cffi binding of the
 * reference would bind.
 *
 * Conventions
 *   - Plain C types only.  All pointers are DEVICE pointers unless named host_*.
 *   - The caller allocates every input, output and workspace buffer.
 *   - Every call is stream-ordered on `stream` (a hipStream_t passed as void*);
 *     nothing synchronises the device except where a function says so.
 *   - Every entry point that takes a `stream` works on that stream's device:
 *     its kernels, their dynamic-LDS grants, the grid sizing (CU count,
 *     occupancy) and any internal allocation use it.  The caller need not make
 *     that device current, and its current device is restored on return.
 *   - Return 0 on success or a negative BEAST_E_* code; beast_last_error()
 *     returns a thread-local message for the last failure.  No C++ exception
 *     crosses this boundary.
 *   - Layouts: params are [B][D*N] "(d n)" order, tokens are [B][N*D] "(n d)"
 *     order, exactly as beast/beast_bspline_tokenizer.py:418-422 produces them.
 *     The DoF order d is joint_indices ++ gripper_indices (:70, :414); the
 *     first n_joint DoFs use basis kind 0 (degree p), the rest kind 1
 *     (degree 0 gripper basis, :88-96).
 */
#ifndef BEAST_HIP_H
#define BEAST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BEAST_OK 0
#define BEAST_E_INVALID (-1)     /* bad argument (maps to ValueError)          */
#define BEAST_E_HIP (-2)         /* HIP runtime / launch failure (RuntimeError) */
#define BEAST_E_UNSUPPORTED (-3) /* shape outside the kernels' envelope       */
#define BEAST_E_WORKSPACE (-4)   /* workspace too small                       */

#define BEAST_ABI_VERSION 6   /* 2: beast_xent_rows, beast_xent_rows_bwd; 3: beast_sample_rows;
                                 4: beast_score_rows, beast_score_rows_bwd; 5: beast_encode_windows_f32;
                                 6: beast_reconstruct_windows_f32, beast_blend_candidates_host,
                                    beast_blend_member_host */

int beast_abi_version(void);
const char* beast_last_error(void);

/* Process-wide tuning / test options.  BEAST_OPT_GENERIC_KERNELS = 1 makes encode and
 * reconstruct use their runtime-shape kernels even where a shape-specialised kernel
 * exists (the BEAST defaults T = 50, N = 10, D = 7 / 14); results are identical.
 * BEAST_OPT_BLOCK_WAVES = 4 or 7 forces the workgroup width of the specialised 14-DoF
 * kernels, 8 forces the per-trajectory kernels (16 waves since round 6; 0 = chosen by batch size); results are
 * identical.
 * BEAST_OPT_MERGE_LDS_MIN = n: BPE merges of pairs counted >= n privatise their pair-count deltas
 * in LDS (default 4096; below, global atomics); results are identical.
 * BEAST_OPT_BPE_ENCODE_MODE = m (tests, measurements): beast_bpe_encode_rows' per-word merge by
 * rounds (0, the default) or by HF's min-heap (1); m + 2 also launches one workgroup per 4 rows
 * instead of only the resident ones.  Results are identical.
 * BEAST_OPT_BPE_DEDUP_KEY_BITS = k (tests): beast_bpe_encode_rows_words keeps only k bits of its
 * 32-bit word hashes, so different words share hashes; the code-point compare behind every hash
 * match keeps them apart (same ids).
 * BEAST_OPT_BPE_TRAIN_HOST_LOOP = 1 (tests): beast_bpe_train runs the host-driven loop at any Vt;
 * 2 reruns it after the batched loop as a string-hash collision would.  Results are identical.
 * BEAST_OPT_LAST_CODEC_LAUNCH (tests, tools; read-only: beast_set_option returns BEAST_E_INVALID):
 * which kernel the last beast_encode_f32 / beast_encode_list_f32 / beast_reconstruct_f32 launch of
 * this process chose, 0 before any launch.  Packed:
 *   bits  0-3   kernel family: 1 k_encode_v, 2 k_encode specialised, 3 k_encode runtime-shape,
 *               4 k_reconstruct_v, 5 k_reconstruct specialised, 6 k_reconstruct runtime-shape (MFMA),
 *               7 k_reconstruct_rows
 *   bits  4-8   trajectories per tile          bits 9-13  waves per workgroup
 *   bits 14-16  KS, MFMA K-steps over the basis functions (reconstruct; 0 otherwise)
 *   bit 17      encode input by contiguous DMA (0: gathered through the strides)
 *   bit 18      reconstruct basis operands in registers (0: in LDS, or read per row from memory)
 *   bit 19      output staged through LDS (0 only for k_reconstruct_rows' direct stores)
 *   bit 20      latency variant (write-through stores, one tile per CU) rather than the bulk one
 * BEAST_OPT_LAST_LAUNCH_GRID (tests; read-only): gridDim.x of the last kernel this process launched
 * through the library, whichever entry point started it; 0 before any launch.  A test reads it
 * right after a call to prove that the persistent kernel it means to check walked several tiles.
 * Options are process-wide and not synchronised: set them before launching, not concurrently. */
#define BEAST_OPT_GENERIC_KERNELS 1
#define BEAST_OPT_BLOCK_WAVES 2
#define BEAST_OPT_MERGE_LDS_MIN 3
#define BEAST_OPT_BPE_ENCODE_MODE 5
#define BEAST_OPT_BPE_DEDUP_KEY_BITS 6
#define BEAST_OPT_BPE_TRAIN_HOST_LOOP 7
#define BEAST_OPT_LAST_CODEC_LAUNCH 8
#define BEAST_OPT_LAST_LAUNCH_GRID 9
int beast_set_option(int option, int value);
/* the option's current value (BEAST_E_INVALID for an unknown option) */
int beast_get_option(int option);

/* ---------------------------------------------------------------- H1/H2 ---
 * Replaces UniBSplineBasis.basis (MP_lite_PyTorch/mp_pytorch/basis_gn/
 * uni_bspline_basis.py:59-113) with LinearPhaseGenerator.phase
 * (phase_gn/linear_phase.py:22-24): basis_out[i][n] = B_{n,degree}(clip((t_i -
 * delay)/tau, 0, 1)) by the same Cox-de Boor recursion, same fp32 op order.
 * knots: [n_knots] with n_knots == degree + 1 + num_basis.  degree <= 8. */
int beast_bspline_basis_f32(const float* times, int64_t n_times, float tau, float delay,
                            const float* knots, int n_knots, int degree, int num_basis,
                            float* basis_out, void* stream);

/* The order-th TIME derivative of the same basis, over the SAME control points:
 * basis_out[i][n] = d^order/dt^order B_{n,degree}(u) at u = clip((t_i - delay)/tau, 0, 1), so
 * derivative = basis_out . params with no control-point differencing.  It stands in for
 * UniBSplineBasis.vel_basis / acc_basis with velocity_control_points /
 * acceleration_control_points (basis_gn/uni_bspline_basis.py:115-190), which
 * UniformBSpline.get_traj_vel / get_traj_acc (mp/uni_bspline.py:299-459) combine:
 *   D1[n] = (degree/tau) (B_{n,degree-1}(u)/(k[n+degree]-k[n]) - B_{n+1,degree-1}(u)/(k[n+degree+1]-k[n+1]))
 * with zero-denominator terms dropped; order 2 applies the rule once more (span degree-1, a
 * second 1/tau): the exact second derivative, NOT get_traj_acc's value, which is that times
 * tau (degree-1)/degree on uniform knot spans.  order 0 runs beast_bspline_basis_f32's kernel (same
 * bits); order in 0..2; order > degree gives zeros.  The phase is clipped first, so outside
 * [delay, delay+tau] the boundary's one-sided derivative is returned; at an interior knot where
 * the derivative jumps (order == degree) the value is the right-continuous one (spans
 * [k_i, k_{i+1}), the last one closed: the reference's degree-0 rule). */
int beast_bspline_basis_deriv_f32(const float* times, int64_t n_times, float tau, float delay,
                                  const float* knots, int n_knots, int degree, int num_basis,
                                  int order, float* basis_out, void* stream);

/* Ridge projection P = (Phi^T Phi + reg I)^-1 Phi^T in float64: the closed form
 * of UniformBSpline.learn_mp_params_from_trajs (mp/uni_bspline.py:539-586) for
 * init/end condition order 0, where the block-diagonal system of
 * basis_multi_dofs (basis_gn/uni_bspline_basis.py:349-356) decouples per DoF.
 * Written zero-padded as proj_out[16][Tp], Tp = round_up(T, 4) (the MFMA A-operand
 * layout of beast_encode_f32).  One workgroup; N <= 16. */
int beast_bspline_projection_f64(const float* basis, int T, int N, double reg, double* proj_out,
                                 void* stream);

/* ------------------------------------------------------------- H4 + H5 ---
 * Replaces BEASTBsplineTokenizer.encode (beast/beast_bspline_tokenizer.py:
 * 399-428) -> learn_mp_params_from_trajs + clamp + continuous_to_discrete
 * (beast/utils.py:4-17) + rearrange + LLM offset, as ONE fused kernel.
 *   traj[b*sb + t*st + dof_src[d]*sd]  fp32 input, element strides
 *   row_elems   size of the input's last dim (for the contiguous fast path)
 *   proj        [2][16][Tp] fp32 zero-padded projections (kind 0 joint, kind 1
 *               gripper): the round-to-nearest fp32 image of the float64 output of
 *               beast_bspline_projection_f64, converted once per time grid
 *   params_out  [B][D*N] fp32 unclamped fit (params_dict['params']); nullable
 *   tokens_out  [B][N*D] int64 = round_half_even(clamp01((clamp(p)-wmin)/max(wmax-wmin,1e-8))*(vocab-1))
 *               + tok_offset; nullable.  vocab <= 0 disables quantisation.
 * Constraints: N <= 16, T <= 256, D <= 64; every shape inside them encodes, at any strides and
 * alignment (16-byte aligned contiguous rows of at most 32 KB per trajectory take the DMA path). */
int beast_encode_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd, int row_elems,
                     int D, int n_joint, const int32_t* dof_src, const float* proj, int N,
                     const float* w_min, const float* w_max, int vocab, int64_t tok_offset,
                     float* params_out, int64_t* tokens_out, void* stream);

/* Params-only fit of a LIST of batches in one launch (fit_parameters, reference :181-220,
 * which fits every dataloader batch then takes quantiles): batch i's rows start at the
 * device pointer traj_list[i] (traj_list itself is a device array of nbatch pointers, each
 * 16-byte aligned), every batch has rows_per_batch (a multiple of 8) contiguous rows of
 * [T][row_elems] fp32; params_out [nbatch * rows_per_batch][D*N] (d n).  Same kernel and
 * arithmetic as beast_encode_f32, so params are bitwise those of per-batch calls. */
int beast_encode_list_f32(const float* const* traj_list, int nbatch, int64_t rows_per_batch, int T, int row_elems,
                          int D, int n_joint, const int32_t* dof_src, const float* proj, int N, float* params_out,
                          void* stream);

/* Quantise-only epilogue of the above for already-fitted params [B][D*N] (d n):
 * used by encode(update_bounds=True) after the bounds move (:415-420).
 * mode 0: tokens_out int64 [B][N*D] (continuous_to_discrete + offset);
 * mode 1: ntok_out fp32 [B][N*D] = normalize_tensor (beast/utils.py:29-35),
 *         the encode_continuous path (:430-450). */
int beast_quantize_f32(const float* params, int64_t B, int D, int N, const float* w_min, const float* w_max,
                       int vocab, int64_t tok_offset, int mode, int64_t* tokens_out, float* ntok_out, void* stream);

/* Fit + quantise on PER-TRAJECTORY time grids with sample weights, one launch: what
 * UniformBSpline.learn_mp_params_from_trajs (mp/uni_bspline.py:471-602) computes when its
 * `times` [*add_dim, T] differ from row to row (init / end condition order 0), extended by a
 * weight per sample, followed by beast_encode_f32's clamp, quantiser, (d n) -> (n d) and offset.
 * Per trajectory b and kind (kind 0: the first n_joint DoFs at `degree`; kind 1: the rest at
 * degree 0), with Phi[t][n] = B_n(clip((times[t] - delay) / tau, 0, 1)), to the bit what
 * beast_bspline_basis_f32 gives for these times:
 *   G = Phi^T diag(w) Phi + reg I,  R = Phi^T diag(w) Y,  params = G^-1 R
 * G, R and the solve (Gauss-Jordan, partial pivoting) are float64; params are rounded to fp32
 * once.  No shared projection is involved: every trajectory has its own Gram matrix.
 *   traj[b*sb + t*st + dof_src[d]*sd]  fp32 input, element strides (as beast_encode_f32)
 *   times       [T] per trajectory, batch stride times_sb (0: one row shared by all)
 *   weights     nullable (all ones): [T] per trajectory >= 0, batch stride weights_sb (0: shared).
 *               WEIGHT 0 SKIPS THE SAMPLE: its time and its values are not used at all and may
 *               be NaN / inf (the mark of a missing frame).  A trajectory whose weights are
 *               all 0 gets params exactly 0.  Negative or non-finite weights are undefined.
 *   knots_joint [degree + 1 + N], knots_grip [1 + N]: the two kinds' knot vectors (each
 *               required only when its kind has DoFs); reg: the ridge term (the reference's 1e-9)
 *   params_out  [B][D*N] fp32 (d n), nullable; tokens_out [B][N*D] int64 (n d), nullable: bitwise
 *               beast_quantize_f32 (mode 0) of params_out; needs w_min, w_max, vocab >= 2.
 * BEAST_E_INVALID: a null required pointer, B < 0, T < 1, N < 1, D < 1, n_joint outside
 * [0, D], a negative stride, a knot count other than the above.  BEAST_E_UNSUPPORTED outside
 * beast_encode_f32's envelope: N <= 16, T <= 256, D <= 64, degree <= 8 (any strides). */
int beast_encode_rows_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd, int D,
                          int n_joint, const int32_t* dof_src, const float* times, int64_t times_sb,
                          const float* weights, int64_t weights_sb, float tau, float delay,
                          const float* knots_joint, int n_knots_joint, const float* knots_grip,
                          int n_knots_grip, int degree, int N, double reg, const float* w_min,
                          const float* w_max, int vocab, int64_t tok_offset, float* params_out,
                          int64_t* tokens_out, void* stream);

/* beast_encode_f32 on WINDOWS of a flat frame buffer, one launch, without materialising them:
 * what a dataset of episodes feeds the tokenizer (LeRobot's rule: the next T actions from a
 * frame, the episode's last frame repeated past its end).
 *   frames[r*sr + c*sd]   fp32 [R][row_elems], element strides; a row ends before the next
 *                         begins (sr >= (row_elems-1)*sd + 1), so all of it lies below frames + R*sr
 *   win_start, win_end    DEVICE int64 [W]: window w covers rows win_start[w] .. win_end[w] - 1 and
 *                         its sample t (0 <= t < T) is row min(win_start[w] + t, win_end[w] - 1)
 * followed by exactly beast_encode_f32 (projection, clamp, quantiser, (d n) -> (n d), offset):
 * params_out [W][D*N] and tokens_out [W][N*D] are bitwise those of beast_encode_f32 on the gathered
 * [W][T][row_elems] tensor.  proj, dof_src, w_min / w_max, vocab, tok_offset and the nullable
 * outputs mean what they mean there; a dof_src entry outside [0, row_elems) is clamped into the
 * row on either path below (as beast_encode_f32's contiguous path does).
 * The tables are not trusted: the kernel clamps win_start into [0, R-1] and win_end into
 * [win_start+1, R], so nothing outside frames[0 .. R*sr) is read whatever they hold (a bad table
 * gives wrong numbers, never a fault).
 * One workgroup takes a tile of consecutive windows.  Where the rows the tile's windows cover
 * (min start .. max min(start+T, end)) number at most tile * T and sd == 1, they are staged in LDS
 * once and shared by the windows (a dense stride-1 table reads every frame about once, not T
 * times); otherwise the tile's windows are gathered one by one.  Same result either way.
 *   tile_counts  nullable uint32[2], zeroed by the caller: += 1 per tile to [0] (shared segment)
 *                or [1] (gathered); for tests and tools.
 * BEAST_E_INVALID: a null required pointer, both outputs null, R < 1 with W > 0, W < 0, T < 1,
 * N < 1, D < 1, row_elems < 1, n_joint outside [0, D], a negative stride, overlapping rows,
 * tokens_out with vocab < 2 or without bounds.  BEAST_E_UNSUPPORTED outside beast_encode_f32's
 * envelope: N <= 16, T <= 256, D <= 64.  W == 0 is a no-op. */
int beast_encode_windows_f32(const float* frames, int64_t R, int64_t sr, int64_t sd, int row_elems,
                             const int64_t* win_start, const int64_t* win_end, int64_t W, int T,
                             int D, int n_joint, const int32_t* dof_src, const float* proj, int N,
                             const float* w_min, const float* w_max, int vocab, int64_t tok_offset,
                             float* params_out, int64_t* tokens_out, uint32_t* tile_counts, void* stream);

/* The way back: blend the tokens of a window table into the rows of a flat [R] frame buffer, one
 * launch, no [W][T][D] intermediate and no atomic on an output.
 *   win_start, win_end  DEVICE int64 [W], the table beast_encode_windows_f32 takes, same meaning:
 *                       window w has rows_w = min(T, end_w - start_w) real samples, sample t < rows_w
 *                       lies on row start_w + t; samples t >= rows_w are edge padding and contribute
 *                       to nothing.  REQUIRED: win_start is non-decreasing (equal starts allowed).
 *   tokens              int64 [W][N*D] in (n d) order, tok_offset subtracted first; or
 *   ntokens             fp32 normalised [W][N*D] in [-1, 1], as beast_reconstruct_f32 reads them
 *                       (exactly one of the two is given)
 *   basis               [2][T][N] fp32, the default-grid basis per kind; w_min / w_max, dof_dst,
 *                       num_dof_out as in beast_reconstruct_f32
 *   blend               fp32 [T], finite and >= 0: the weight of sample index t
 * y_w(t, d) is window w's reconstruction: coefficients decoded bit-exactly as beast_reconstruct_f32
 * decodes them, then ONE fma chain over the N basis functions starting from 0 against the basis
 * row of the DoF's kind, in the order beast_reconstruct_f32 sums them for the same N, T, D,
 * num_dof_out and token form (on the matrix cores n = k*KS + ks for ks = 0 .. KS-1, k = 0 .. 3 with
 * KS = ceil(N/4); n ascending where that entry point takes its per-row kernel), so y_w(t, d) is
 * bitwise what beast_reconstruct_f32 writes for window w's tokens alone.  For row r and DoF d let
 * w_1 < w_2 < ... < w_C be the windows, in TABLE ORDER, with start_w <= r < start_w + rows_w and
 * blend[r - start_w] != 0, and t_k = r - start_{w_k}:
 *     num = 0; den = 0
 *     for k = 1 .. C:  num = fmaf(blend[t_k], y_{w_k}(t_k, d), num);  den = den + blend[t_k]
 *     frames_out[r*out_sr + dof_dst[d]] = C > 0 ? num / den (IEEE division) : fill
 *     coverage_out[r] = C (int32)        weight_out[r] = den (fp32; 0 where C = 0)
 * A sample whose blend weight is 0 is skipped, not multiplied (a NaN there does not propagate).  The
 * columns of frames_out[r][0 .. num_dof_out) dof_dst does not name are written 0; every element of
 * the three outputs is written (they may be uninitialised).  A row's value depends only on its own
 * contributors and their table order: not on R, W, the tiling or the rest of the table, and two
 * runs agree bitwise.
 * The tables are not trusted: starts are clamped into [0, R-1] and ends into [start+1, R] as
 * beast_encode_windows_f32 clamps them, and the candidate search reads table indices in [0, W)
 * only, so a bad device table (out of range, or not sorted: windows are then missed) gives wrong
 * numbers, never a fault.
 *   coverage_out, weight_out  nullable
 *   tile_counts  nullable uint32[2], zeroed by the caller: per tile of output rows, [0] += the
 *                chunks of candidate windows walked, [1] += 1 if more than one; for tests and tools.
 * BEAST_E_INVALID: a null required pointer, both or neither of tokens / ntokens, W < 0, R < 0,
 * T < 1, N < 1, D < 1, n_joint outside [0, D], num_dof_out < D, out_sr < num_dof_out, tokens with
 * vocab < 2.  BEAST_E_UNSUPPORTED outside N <= 16, T <= 256, D <= 64, num_dof_out <= 4096.
 * R == 0 is a no-op; W == 0 with R > 0 is not (every row gets fill, 0, 0; the table and token
 * pointers are then never read). */
int beast_reconstruct_windows_f32(const int64_t* tokens, const float* ntokens, int64_t W, int D, int n_joint,
                                  int N, int vocab, int64_t tok_offset, const float* w_min, const float* w_max,
                                  const float* basis, int T, const int64_t* win_start, const int64_t* win_end,
                                  int64_t R, const float* blend, float fill, const int32_t* dof_dst,
                                  int num_dof_out, float* frames_out, int64_t out_sr, int32_t* coverage_out,
                                  float* weight_out, uint32_t* tile_counts, void* stream);

/* Host only, no GPU: beast_reconstruct_windows_f32's index logic (csrc/blend_index.h) over HOST
 * arrays, for tests.  beast_blend_candidates_host: the half-open range [a, b) of windows that can
 * own a row of [r0, r1), 0 <= r0 <= r1 <= R: a is the first w whose (clamped) start exceeds r0 - T,
 * b the first whose start is >= r1, by binary search; 0 <= *a_out <= *b_out <= W and every table
 * index read lies in [0, W) whatever the table holds (win_end is part of the table but no search
 * reads it).  beast_blend_member_host: the sample index t in [0, T) as which the window
 * (start, end), clamped, owns row r, or -1 where it does not (or R < 1, T < 1). */
int beast_blend_candidates_host(const int64_t* win_start, const int64_t* win_end, int64_t W, int64_t R, int T,
                                int64_t r0, int64_t r1, int64_t* a_out, int64_t* b_out);
int beast_blend_member_host(int64_t start, int64_t end, int64_t R, int T, int64_t r);

/* ------------------------------------------------------------- H6 - H8 ---
 * Replaces BEASTBsplineTokenizer.decode + reconstruct_traj (beast/
 * beast_bspline_tokenizer.py:483-536) -> discrete_to_continuous (beast/
 * utils.py:20-26), optional init_p overwrite of coefficient 0 of the joint
 * DoFs (:505-510), UniformBSpline.get_traj_pos (mp/uni_bspline.py:114-177)
 * and the scatter to joint/gripper columns (:520-534).
 *   tokens      [B][N*D] int64 (tok_offset is SUBTRACTED first)
 *   basis       [2][T_out][N] fp32 per kind; batch stride basis_sb (0 = shared)
 *   dof_dst     [D] output column of each DoF (D distinct columns); pos_out [B][T_out][num_dof_out],
 *               num_dof_out >= D: the columns dof_dst does not name are written as 0
 *   init_p      nullable [B] rows of stride init_p_sb; init_p_src[d] column for
 *               joint DoF d (< n_joint)
 *   params_out  nullable [B][D*N] decoded params (= decode()); pos_out nullable.
 *   ntokens     nullable: when set, fp32 normalised tokens [B][N*D] in [-1, 1] are
 *               read instead of `tokens` and mapped back by denormalize_tensor
 *               (beast/utils.py:38-44): the reconstruct_traj_continuous path (:538-582). */
int beast_reconstruct_f32(const int64_t* tokens, int64_t B, int D, int n_joint, int N, int vocab,
                          int64_t tok_offset, const float* w_min, const float* w_max,
                          const float* basis, int64_t basis_sb, int T_out,
                          const int32_t* dof_dst, int num_dof_out,
                          const float* init_p, int64_t init_p_sb, const int32_t* init_p_src,
                          float* params_out, float* pos_out, const float* ntokens, void* stream);

/* Positions, velocities and accelerations from tokens in ONE launch: what
 * UniformBSpline.get_traj_pos / get_traj_vel / get_traj_acc (mp/uni_bspline.py:114-177,
 * :299-459) give for the decoded params, with the acceleration being the exact second time
 * derivative (see beast_bspline_basis_deriv_f32).  Every argument means what it means in
 * beast_reconstruct_f32 (token order (n d), tok_offset subtracted, ntokens, init_p, dof_dst,
 * unnamed output columns written 0), except:
 *   basis       [3][2][T_out][N] fp32, order-major: slab o holds the order-o basis of kind 0
 *               (joint) and kind 1 (gripper); basis_sb = 0 (shared) or a per-trajectory stride
 *               covering all three slabs.  The slab of a null output is never read (it may be
 *               unallocated, as long as the used slabs sit at their order's offset).
 *   pos_out, vel_out, acc_out   [B][T_out][num_dof_out] each; nullable, at least one given.
 *               Gripper DoFs (d >= n_joint, degree 0) get 0 in vel_out and acc_out whatever
 *               their slab holds.
 * Tokens are read and dequantised once per trajectory; every requested order is written from
 * that copy.  N <= 16, D <= 64, T_out <= 4096, num_dof_out <= 4096, else BEAST_E_UNSUPPORTED. */
int beast_reconstruct_derivs_f32(const int64_t* tokens, int64_t B, int D, int n_joint, int N, int vocab,
                                 int64_t tok_offset, const float* w_min, const float* w_max,
                                 const float* basis, int64_t basis_sb, int T_out,
                                 const int32_t* dof_dst, int num_dof_out,
                                 const float* init_p, int64_t init_p_sb, const int32_t* init_p_src,
                                 float* pos_out, float* vel_out, float* acc_out, const float* ntokens,
                                 void* stream);

/* The adjoint of beast_reconstruct_derivs_f32 on its ntokens path, in ONE launch: upstream
 * gradients of the positions, velocities and accelerations -> the gradient of the normalised
 * tokens (and of init_p).  B .. num_dof_out, basis_sb and init_p_src mean what they mean in the
 * forward.  With k = d*N + n, kind(d) = 0 for d < n_joint else 1, o over the non-null gradients
 * (gripper DoFs: o = 0 only) and x = ntokens[b][n*D+d]:
 *   S[b][d][n]              = sum_t sum_o basis_o[kind(d)][t][n] * grad_o[b][t][dof_dst[d]]
 *   grad_ntokens[b][n*D+d]  = (-1 <= x <= 1) ? S[b][d][n] * s[k] : 0,   s[k] = 0.5f * (w_max[k] - w_min[k])
 * s is the exact derivative of denormalize_tensor; both ends of the clamp pass, as in torch's
 * clamp backward; the mask is a select, so an x outside the range or NaN gives exactly 0 even
 * where S is not finite.
 *   grad_pos, grad_vel, grad_acc   [B][T_out][num_dof_out] fp32, contiguous; nullable, at least
 *               one given.  Columns dof_dst does not name contribute nothing.
 *   basis       the forward's slabs [3][2][T_out][N]; the slab of a null gradient is never read.
 *               For beast_reconstruct_f32's [2][T_out][N] basis pass it with grad_pos alone.
 *   ntokens     [B][N*D]: the forward's input (the clamp mask)
 *   init_p_src  nullable; non-null means the forward ran with init_p: grad_ntokens is 0 for
 *               coefficient 0 of the joint DoFs (the forward overwrote it), and
 *   grad_init_p nullable (needs init_p_src) [B] rows of stride grad_init_p_sb, zero-filled by the
 *               caller: grad_init_p[b][init_p_src[d]] = S[b][d][0] for d < n_joint; no other
 *               column is written.
 *   grad_ntokens  required [B][N*D] (n d), every element written
 * No atomics: every S is one fma chain over t ascending and, inside each t, o ascending,
 * whatever B, the tile or the launch variant, so two runs agree bitwise and a row's gradient
 * does not depend on the batch around it.  Each gradient is read once (16-byte loads where the
 * three pointers and T_out*num_dof_out allow them).  Same envelope as the forward:
 * N <= 16, D <= 64, T_out <= 4096, num_dof_out <= 4096, else BEAST_E_UNSUPPORTED. */
int beast_reconstruct_derivs_bwd_f32(const float* grad_pos, const float* grad_vel, const float* grad_acc,
                                     int64_t B, int D, int n_joint, int N,
                                     const float* w_min, const float* w_max,
                                     const float* basis, int64_t basis_sb, int T_out,
                                     const int32_t* dof_dst, int num_dof_out,
                                     const float* ntokens, const int32_t* init_p_src,
                                     float* grad_ntokens, float* grad_init_p, int64_t grad_init_p_sb,
                                     void* stream);

/* Decode from logits: the bridge from a discrete head's logits to the normalised coefficients
 * that beast_reconstruct_f32 / beast_reconstruct_derivs_f32 take as `ntokens` (and
 * beast_reconstruct_derivs_bwd_f32 differentiates).  The reference has no counterpart.  For one
 * token row l[0..V) (token k = n*D + d of trajectory b) and tau = temperature > 0:
 *   z_v  = l_v / tau      zmax = max_v z_v      e_v = exp(z_v - zmax)      s = sum_v e_v
 *   mean = clamp(sum_v e_v * x_v / s, -1, 1),   x_v = 2v/(V-1) - 1
 *   amax = the lowest v with l_v == max_v l_v   (on the raw logits: no rounding enters)
 *   grad_l_v = (g / tau) * (e_v / s) * (x_v - mean)      (g: the upstream gradient of mean)
 * In exact arithmetic mean lies in [-1, 1]; the clamp only removes an fp32 overshoot (which the
 * mask of beast_reconstruct_derivs_bwd_f32 would turn into a zero gradient) and its derivative is
 * taken as 1.  A -inf entry has probability exactly 0 and gradient exactly 0.  A row that holds a
 * NaN or +inf, or only -inf, yields unspecified values in ITS OWN outputs; it does not fault and
 * does not disturb any other row.  Arithmetic is fp32 whatever the element type.  Where one bin
 * holds the mass, x_v - mean cancels; the backward therefore measures x_v and the mean from the
 * bin nearest to the forward's mean (exact integers, one more sum over the row), so a peaked row's
 * gradient keeps its relative accuracy instead of inheriting the rounding of the fp32 mean.
 *   logits      [B][K][V] of `dtype` (BEAST_LOGITS_*), element strides sb, sk >= 0; the V axis has
 *               stride 1.  Each row is read from memory ONCE per direction, for every V, with
 *               16-byte loads where the row's own address is 16-byte aligned and element loads
 *               where it is not (alignment is a per-row property: a bf16 slice with a 600-byte row
 *               stride alternates).
 *   tok_offset  added to amax (the LLM-vocabulary offset, as in beast_encode_f32)
 *   mean_out    nullable [B][K]     normalised, in [-1, 1]
 *   argmax_out  nullable [B][K]     amax + tok_offset
 *   stats_out   nullable [B][K][2]  (zmax, s): the backward's input
 *   At least one of the three outputs is non-null.
 *   grad_mean   [B][K] contiguous;  mean, stats: what the forward wrote for the same logits
 *   grad_logits [B][K][V] of `dtype`, element strides gsb >= 0, gsk >= V (rows must not overlap),
 *               V stride 1; every element of every row is written and nothing around it.
 * One wave owns a row; element v always belongs to lane (v / (16 / sizeof(T))) % 64 and every sum
 * has an order fixed by (V, dtype) alone -- no atomics, no LDS -- so a row's outputs are bitwise
 * identical alone or in any batch, at any alignment, in any grid and from run to run.
 * Envelope: 2 <= V <= 65536, else
 * BEAST_E_UNSUPPORTED; temperature must be finite and > 0; B = 0 returns 0 without a launch. */
#define BEAST_LOGITS_F32 0
#define BEAST_LOGITS_F16 1
#define BEAST_LOGITS_BF16 2

int beast_logits_expect(const void* logits, int dtype, int64_t B, int K, int V,
                        int64_t sb, int64_t sk,
                        float temperature, int64_t tok_offset,
                        float* mean_out, int64_t* argmax_out, float* stats_out,
                        void* stream);

int beast_logits_expect_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                            float temperature, const float* mean, const float* stats,
                            const float* grad_mean,
                            void* grad_logits, int64_t gsb, int64_t gsk,
                            void* stream);

/* Rows that one launch of beast_logits_expect (backward != 0: of beast_logits_expect_bwd) keeps
 * resident on the stream's device for this dtype and V: a launch over more rows walks them with a
 * grid stride.  Launches nothing.  Returns the count (> 0) or a negative BEAST_E_* code. */
int64_t beast_logits_resident_rows(int dtype, int V, int backward, void* stream);

/* Train a discrete head from its logits: the cross-entropy of a token row against a token, or
 * against the TWO-HOT target of an unquantised normalised coefficient, and its gradient.  The
 * reference has no counterpart.  The bins are ordinal and affine in the coefficient, so the two
 * bins around x, weighted 1-f and f, have expectation exactly x: a head trained on that target is
 * consistent with beast_logits_expect at its optimum.  For one row l[0..V), no temperature:
 *   m = max_v l_v      e_v = exp(l_v - m)      s = sum_v e_v
 *   target position u in [0, V-1]:
 *     from a token t (target_tok, tok_offset subtracted):  u = t
 *     from a coefficient x (target_pos):  u = clamp(((x + 1) * 0.5) * (V-1), 0, V-1), the three
 *     roundings in fp32 in this order
 *   i = min(floor(u), V-2),  f = u - i in [0, 1]
 *   q_v    = (1-eps) [(1-f) (v == i) + f (v == i+1)] + eps / V          (eps = smoothing)
 *   loss   = log s + (1-eps) [(1-f) (m - l_i) + f (m - l_{i+1})] + eps (sum_v (m - l_v)) / V
 *   grad_v = g (e_v / s - q_v)                       (g: the upstream gradient of the row's loss)
 *   amax   = the lowest v with l_v == m, + tok_offset, as beast_logits_expect
 * Every term of the loss is >= 0.  A term whose weight is exactly 0 (f == 0, 1-f == 0, eps == 0)
 * contributes exactly 0 whatever the logit: a -inf logit under a zero weight gives neither NaN nor
 * inf, under a positive weight it gives +inf loss.  A row whose token equals ignore_index (as
 * given, before tok_offset is subtracted) or whose coefficient is NaN is ignored: loss exactly 0
 * and all V gradient elements written as 0.  Any other token outside [tok_offset, tok_offset + V)
 * gives NaN loss and a NaN gradient row; the target is only compared with v, never an address.  A
 * row whose logits hold NaN or +inf, or only -inf, has unspecified outputs of its own and
 * disturbs no other row.
 *   logits       as beast_logits_expect (dtype, strides, one read per direction, alignment)
 *   target_tok   [B][K] contiguous int64, or null   } exactly one of the two
 *   target_pos   [B][K] contiguous fp32, or null    }
 *   smoothing    in [0, 1)
 *   loss_out     nullable [B][K]
 *   stats_out    nullable [B][K][2]  (m, s): the backward's input
 *   argmax_out   nullable [B][K]     amax + tok_offset
 *   At least one of the three outputs is non-null.
 *   grad_loss    [B][K] contiguous;  stats: what the forward wrote for the same logits
 *   grad_logits  [B][K][V] of `dtype`, element strides gsb >= 0, gsk >= V, V stride 1; every element
 *                of every row is written and nothing around it.
 * Rows, lanes and sums are those of beast_logits_expect: a row's outputs are bitwise identical
 * alone or in any batch, at any alignment, in any grid and from run to run.
 * Envelope: 2 <= V <= 65536, else
 * BEAST_E_UNSUPPORTED; B = 0 returns 0 without a launch. */
int beast_xent_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                    const int64_t* target_tok, const float* target_pos,
                    int64_t tok_offset, int64_t ignore_index, float smoothing,
                    float* loss_out, float* stats_out, int64_t* argmax_out,
                    void* stream);

int beast_xent_rows_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                        const int64_t* target_tok, const float* target_pos,
                        int64_t tok_offset, int64_t ignore_index, float smoothing,
                        const float* stats, const float* grad_loss,
                        void* grad_logits, int64_t gsb, int64_t gsk,
                        void* stream);

/* Draw tokens from a discrete head's logits: S inverse-CDF draws per row under
 * softmax(l / temperature), optionally truncated to the top-k and then the top-p (nucleus) bins,
 * with the log-probability of every draw.  The reference has no counterpart.  The library holds no
 * random number generator: the caller owns the uniforms as it owns every other buffer.  For one row
 * l[0..V), z = l / temperature, zmax = max z, e_v = exp(z_v - zmax):
 *   top-k (1 <= top_k < V):  theta_k = the k-th largest value of l, counting multiplicity;
 *     K1 = {v : l_v >= theta_k} -- ties at the k-th value are all kept.  top_k = 0 or >= V: every bin.
 *   top-p (0 < top_p < 1):  S1 = sum_{K1} e;  theta_p = the largest value t among {l_v : v in K1}
 *     with sum_{v in K1, l_v >= t} e_v >= top_p S1;  kept = {v in K1 : l_v >= theta_p} -- the
 *     smallest value-closed set of the most probable bins whose mass reaches top_p; a tie at the
 *     nucleus' edge stays whole.  top_p = 1: kept = K1.
 *   draw:  S2 = sum_kept e;  C_v = sum_{w <= v, w in kept} e_w in ascending index;
 *     tok_s = the lowest kept v with C_v > u_s S2 (the highest kept v with e_v > 0 where rounding
 *     leaves none);  logprob_s = (z_tok - zmax) - log S2, the log-probability under the distribution
 *     drawn from;  kept_count = |kept|.
 * The thresholds compare the raw logits.  A bin with e_v = 0 (a -inf logit) is never drawn; the bin
 * that holds the maximum is always kept.  A row with NaN or +inf, or only -inf, or a uniform that is
 * NaN or outside [0, 1), has unspecified outputs of its own, still writes tokens inside
 * [tok_offset, tok_offset + V) and disturbs no other row.  Nothing is addressed by a computed value.
 *   logits       as beast_logits_expect (dtype, strides, alignment); the row is read once for all S
 *                draws (twice, the second time from L2, beyond four chunks)
 *   uniforms     [S][B][K] contiguous fp32 in [0, 1)
 *   tokens_out   [S][B][K] int64, tok + tok_offset
 *   logprob_out  nullable [S][B][K] fp32
 *   kept_out     nullable [B][K] int32
 * Rows, lanes and sums are those of beast_logits_expect: a row's outputs are bitwise identical alone
 * or in any batch, at any alignment, in any grid and from run to run, and draw s depends on u_s only.
 * Envelope: 2 <= V <= 65536 and
 * 1 <= S <= 64; a truncation (1 <= top_k < V or top_p < 1) only for rows of up to four chunks
 * (V <= 1,024 fp32, V <= 2,048 fp16 / bf16 -- BEAST vocabularies are 256), else BEAST_E_UNSUPPORTED.
 * temperature finite and > 0, top_k >= 0, 0 < top_p <= 1; B = 0 returns 0 without a launch. */
int beast_sample_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                      float temperature, int top_k, float top_p,
                      const float* uniforms, int S, int64_t tok_offset,
                      int64_t* tokens_out, float* logprob_out, int32_t* kept_out,
                      void* stream);

/* Score tokens under a discrete head's logits: the log-probability of S given tokens per row, the
 * entropy of the row's distribution and its divergence from a reference row, with the gradient of
 * all three.  The reference has no counterpart.  For one row l[0..V), temperature, top_k, top_p:
 * z, zmax, e_v, the kept set and S2 are EXACTLY those of beast_sample_rows (thresholds on the raw
 * logits, ties whole, S2 summed in the sampler's order), and
 *   log pi_v = (z_v - zmax) - log S2 for kept v;  pi_v = 0 and log pi_v = -inf outside the kept set
 * so the log-probability of a token beast_sample_rows drew has the bits of its logprob_out.
 *   per draw s < S, token t_s (tok_offset subtracted):  logprob_s = log pi_{t_s}
 *     a token equal to ignore_index (as given, before the offset is subtracted): exactly 0
 *     a token outside the kept set, or on a -inf logit: -inf
 *     any other token outside [tok_offset, tok_offset + V): NaN, and a NaN gradient row
 *     a draw whose logprob is 0 by ignore_index or -inf takes no part in the backward;
 *     a token is only compared with v, never an address
 *   entropy     H  = -sum_kept pi_v log pi_v;  a term with pi_v == 0 is exactly 0 (a select)
 *   kl          KL = sum_kept pi_v (log pi_v - log rho_v),  rho = softmax(ref / temperature) over
 *               ALL V bins, never truncated; pi_v == 0 terms are exactly 0; +inf where
 *               rho_v == 0 < pi_v.  Only with ref_logits.
 *   kept_count  |kept|
 *   backward, upstream g_s, g_H, g_KL, the kept set constant; for kept v
 *     grad_v = (1/temperature) [ sum_s g_s 1[t_s = v] - pi_v sum_s g_s - g_H pi_v (log pi_v + H)
 *                                + g_KL pi_v (log pi_v - log rho_v - KL) ]
 *     the sums over s over the draws that take part; grad_v is exactly 0 outside the kept set and
 *     where pi_v == 0; the reference never receives a gradient.
 * A row with NaN or +inf, or only -inf, in the logits or the reference has unspecified outputs of
 * its own, still writes in bounds and disturbs no other row.
 *   logits        as beast_logits_expect (dtype, strides, alignment); read once per direction
 *                 (twice forward, the second time from L2, beyond four chunks)
 *   ref_logits    nullable; same dtype and V, element strides rsb, rsk >= 0, V stride 1
 *   tokens        [S][B][K] contiguous int64; S = 0: null
 *   logprob_out   nullable [S][B][K] fp32; needs S >= 1
 *   entropy_out   nullable [B][K]
 *   kl_out        nullable [B][K]; needs ref_logits
 *   kept_out      nullable [B][K] int32
 *   stats_out     nullable [B][K][10], the backward's input:
 *                 [0] zmax  [1] S2  [2] the lowest kept raw logit (-inf without a truncation): the
 *                 backward's kept set is {l_v >= it}, no threshold search  [3] H  [4] KL (0 without
 *                 ref_logits)  [5], [6] the reference's zmax and sum (0 without)  [7] 0
 *                 [8], [9] the low and high 32 bits, as bit patterns, of the mask of the draws that
 *                 take part in the backward
 *   At least one of the five outputs is non-null.
 *   stats         what the forward wrote for the same inputs
 *   grad_logprob  nullable [S][B][K]; needs S >= 1   } at least one of the three;
 *   grad_entropy  nullable [B][K]                    } the backward reads each logits row once, and
 *   grad_kl       nullable [B][K]; needs ref_logits  } the reference row only with grad_kl
 *   grad_logits   [B][K][V] of `dtype`, element strides gsb >= 0, gsk >= V, V stride 1; every element
 *                 of every row is written and nothing around it.
 * Rows, lanes and sums are those of beast_logits_expect: a row's outputs are bitwise identical alone
 * or in any batch, at any alignment, in any grid and from run to run.
 * Envelope: beast_sample_rows' -- 2 <= V <=
 * 65536 and 0 <= S <= 64; a truncation (1 <= top_k < V or top_p < 1) only for rows of up to four
 * chunks (V <= 1,024 fp32, V <= 2,048 fp16 / bf16), else BEAST_E_UNSUPPORTED.  temperature finite
 * and > 0, top_k >= 0, 0 < top_p <= 1; B = 0 returns 0 without a launch. */
int beast_score_rows(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                     const void* ref_logits, int64_t rsb, int64_t rsk,
                     float temperature, int top_k, float top_p,
                     const int64_t* tokens, int S, int64_t tok_offset, int64_t ignore_index,
                     float* logprob_out, float* entropy_out, float* kl_out, int32_t* kept_out, float* stats_out,
                     void* stream);

int beast_score_rows_bwd(const void* logits, int dtype, int64_t B, int K, int V, int64_t sb, int64_t sk,
                         const void* ref_logits, int64_t rsb, int64_t rsk,
                         float temperature, int top_k, float top_p,
                         const int64_t* tokens, int S, int64_t tok_offset, int64_t ignore_index,
                         const float* stats,
                         const float* grad_logprob, const float* grad_entropy, const float* grad_kl,
                         void* grad_logits, int64_t gsb, int64_t gsk,
                         void* stream);

/* Error statistics of encode -> reconstruct in ONE launch: how well the tokenizer represents the
 * trajectories, and whether the spline fit or the quantiser is to blame.  traj .. dof_src, proj,
 * N, w_min, w_max, vocab and tok_offset mean what they mean in beast_encode_f32; basis is
 * beast_reconstruct_f32's shared grid [2][T][N] (basis_sb = 0, T_out = T).  With
 * y[t] = traj[b][t][dof_src[d]], stats_out[b][d] (DoF order d = joint ++ gripper) holds
 *   [0] sum_t e_t   [1] sum_t e_t^2   [2] max_t |e_t|   [3] sum_t f_t^2
 * where e_t = y[t] - pos[t]: pos is, to the bit, what beast_reconstruct_f32 (no init_p) returns
 * for the tokens beast_encode_f32 produces from this trajectory; and f_t = y[t] - fit[t]: fit is
 * the same reconstruction of the unclamped, unquantised params (the bits of encode's
 * params_out), i.e. the error of the spline fit alone.  The sums run in a fixed order (results
 * are run-to-run identical); the maximum propagates NaN as torch.amax does, so a NaN sample makes
 * all four values of its DoF NaN and leaves the other DoFs alone.
 *   tokens_out   nullable [B][N*D]: exactly beast_encode_f32's tokens
 *   stats_out    required [B][D][4] fp32
 *   clip_counts  nullable uint32 [2][D*N] in (d n) order, ADDED to (the caller zero-fills):
 *                [0] counts the trajectories whose param is < w_min, [1] those > w_max (NaN in
 *                neither); one integer atomic per non-zero column and workgroup, so exact
 * Same envelope as beast_encode_f32 (N <= 16, T <= 256, D <= 64, vocab >= 2, any strides and
 * alignment); w_min and w_max are required.  The trajectory is read once (2,800 B at the default
 * shape) and 16 B per (b, d) are written, plus the tokens if asked. */
int beast_roundtrip_stats_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                              int row_elems, int D, int n_joint, const int32_t* dof_src,
                              const float* proj, const float* basis, int N,
                              const float* w_min, const float* w_max, int vocab, int64_t tok_offset,
                              int64_t* tokens_out, float* stats_out, uint32_t* clip_counts, void* stream);

/* ---------------------------------------------------- §8f rank 4: conditions ---
 * init_cond_order / end_cond_order != 0 (init_order in 0..2, end_order in -1..2, not both 0).
 * beast_cond_fixed_f32 replaces the per-fit condition step of UniBSpline.learn
 * (MP_lite_PyTorch/mp_pytorch/mp/uni_bspline.py:499-550 calling compute_init_params /
 * compute_end_params, basis_gn/uni_bspline_basis.py:192-301): for trajectories traj
 * [B][T][*] (element strides sb, st, sd) and the joint DoFs joint_idx[dj], with
 * dt = times[1] - times[0] and the knot steps knots[1+degree] - knots[1] /
 * knots[n_ctrl-1+degree] - knots[n_ctrl-1] of the joint spline (n_ctrl control points):
 *   init_pos, init_vel [B][dj], params_init [B][dj][init_order]   (init_order > 0)
 *   end_pos, end_vel [B][dj], params_end [B][dj][|end_order|]     (end_order != 0)
 * in the reference's fp32 op order.  T >= 2.
 * beast_cond_add_f32 replaces the fixed control points' part of UniBSpline.get_traj_pos
 * (uni_bspline.py:126-166): pos [B][T][D] (contiguous, the fitted columns' positions from
 * beast_reconstruct_f32) gains, at the joint DoFs, sum_k full_basis[t][k] * fixed[k] (+ init_pos
 * when init_order > 0) over the fixed columns k (the first init_order, the last |end_order|;
 * end order -1 subtracts params_end from column n_ctrl-2).  full_basis [T][n_ctrl] with
 * full_sb = 0, or per trajectory [B][T][n_ctrl] with full_sb = T * n_ctrl. */
int beast_cond_fixed_f32(const float* traj, int64_t B, int T, int64_t sb, int64_t st, int64_t sd,
                         const int32_t* joint_idx, int dj, const float* times, const float* knots, int degree,
                         int n_ctrl, float tau, int init_order, int end_order, float* init_pos, float* init_vel,
                         float* end_pos, float* end_vel, float* params_init, float* params_end, void* stream);
int beast_cond_add_f32(float* pos, int64_t B, int T, int D, const int32_t* joint_idx, int dj,
                       const float* full_basis, int64_t full_sb, int n_ctrl, int init_order, int end_order,
                       const float* params_init, const float* params_end, const float* init_pos, void* stream);

/* ------------------------------------------------------------------ H13 ---
 * Column min / max with NaN propagation (torch.min/max(dim=0)), used by
 * update_weights_bounds / update_weights_bounds_per_batch (:362-389).
 * workspace >= beast_colminmax_workspace_bytes(rows, cols). */
size_t beast_colminmax_workspace_bytes(int64_t rows, int cols);
int beast_colminmax_f32(const float* x, int64_t rows, int cols, int64_t row_stride, float* out_min,
                        float* out_max, void* workspace, size_t ws_bytes, void* stream);

/* Exact per-column quantiles with numpy 'linear' semantics in float32
 * (np.quantile(params, q, axis=0), :213-214) by radix select on order-preserving keys:
 * radix_bits 11 (three passes: 11/11/10 bits) or 7 (four passes: 11/7/7/7 bits; smaller histograms
 * to all-reduce for one more pass over the keys).  Multi-GPU: call
 * prepare, then for pass in 0 .. beast_quantile_passes(radix_bits) - 1 { hist; all-reduce(SUM,
 * uint32) of the first beast_quantile_hist_count(pass, ...) elements at beast_quantile_hist_ptr;
 * select }, then finalize (every rank selects the same order statistics).  n_total = rows summed
 * over all ranks (< 2^32).  n_q <= 4 (host_q). */
size_t beast_quantile_workspace_bytes(int64_t rows, int cols, int n_q);
int beast_quantile_prepare(const float* x, int64_t rows, int cols, int64_t row_stride, int64_t n_total,
                           int n_q, const float* host_q, void* workspace, size_t ws_bytes, void* stream);
uint32_t* beast_quantile_hist_ptr(void* workspace, int cols, int n_q);
int beast_quantile_passes(int radix_bits);
int64_t beast_quantile_hist_count(int pass, int cols, int n_q, int radix_bits);
/* prepare over a list of row-major segments instead of one matrix (fit_parameters' per-batch
 * params without a concatenation): seg_table = device array of nseg {const float* ptr;
 * int64_t first_row; int64_t row_stride} (24 B each, first_row ascending from 0), rows = the
 * total, max_seg_rows = the largest segment. */
int beast_quantile_prepare_segments(const void* seg_table, int nseg, int64_t max_seg_rows, int64_t rows, int cols,
                                    int64_t n_total, int n_q, const float* host_q, void* workspace, size_t ws_bytes, void* stream);
int beast_quantile_hist(int pass, int64_t rows, int cols, int n_q, int radix_bits, void* workspace, void* stream);
int beast_quantile_select(int pass, int cols, int n_q, int radix_bits, void* workspace, void* stream);
int beast_quantile_finalize(int cols, int n_q, void* workspace, float* out, void* stream);
/* single-GPU convenience: all of the above. out [n_q][cols]. */
int beast_quantile_f32(const float* x, int64_t rows, int cols, int64_t row_stride, int n_q, const float* host_q,
                       float* out, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------ H9 - H12 ---
 * Byte-level BPE training, replacing HF tokenizers' BpeTrainer::do_train as
 * driven by FIGBPE (beast/beast_bpe_trainer.py:61-98).  Tokens are int64 code
 * points (bins); a sequence is tokens[seq_off[s] .. seq_off[s+1]). */
int beast_i64_minmax(const int64_t* x, int64_t n, int64_t* out2, void* stream);
/* present[x - min_tok] = 1 for every token (n_cp = max-min+1); multi-GPU: all-reduce MAX */
int beast_bpe_cp_presence(const int64_t* tok, int64_t n, int64_t min_tok, uint8_t* present, int64_t n_cp,
                          void* stream);
/* GPT-2 ByteLevel pre-tokenisation, pass 1: words and byte-symbols per sequence.
 * cls_lut[cp] in {0 other, 1 letter, 2 number, 3 whitespace}, cp < lut_n. */
int beast_bpe_pretok_count(const int64_t* tok, const int64_t* seq_off, int64_t n_seq, int64_t min_tok,
                           const uint8_t* cls_lut, int64_t lut_n, int64_t* words_per_seq,
                           int64_t* syms_per_seq, void* stream);
/* exclusive scan: out[0..n] (out[n] = total). workspace >= beast_scan_workspace_bytes(n) */
size_t beast_scan_workspace_bytes(int64_t n);
int beast_exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, void* workspace, void* stream);
/* pass 2: emit byte symbols as vocab ids (byte2id[256]) and word extents. */
int beast_bpe_pretok_emit(const int64_t* tok, const int64_t* seq_off, int64_t n_seq, int64_t min_tok,
                          const uint8_t* cls_lut, int64_t lut_n, const int64_t* word_off,
                          const int64_t* sym_off, const uint16_t* byte2id, uint16_t* sym,
                          uint32_t* wstart, uint32_t* wlen, void* stream);
/* pair table [Vt][Vt] uint32 += word count for each adjacent pair (BpeTrainer::count_pairs).
 * n_sym: every symbol id is < n_sym (the setup vocabulary); small n_sym count in LDS. */
int beast_bpe_count_pairs(const uint16_t* sym, const uint32_t* wstart, const uint32_t* wlen,
                          const uint32_t* wcount, int64_t n_words, uint32_t* table, int Vt, int n_sym,
                          void* stream);
/* sig[w] = word w's 64-bit Bloom signature (csrc/bpe_common.h sig_of): the low 32 bits hold its
 * symbols, two bits each (sig_sym), the high 32 its adjacent pairs, two bits each from one hash of
 * the pair (sig_pair); a word of no symbols has signature 0.  A word can hold the adjacent pair
 * (a, b) only if it has every bit of sig_need(a, b) = sig_sym(a) | sig_sym(b) | sig_pair(a, b): the
 * merges skip the other words without reading their symbols, and keep sig current for the words
 * they rewrite. */
int beast_bpe_word_signatures(const uint16_t* sym, const uint32_t* wstart, const uint32_t* wlen, int64_t n_words,
                              uint64_t* sig, void* stream);

/* -- the merge loop (csrc/bpe_loop.hip), replacing the loop of HF BpeTrainer::do_train as called
 * from beast/beast_bpe_trainer.py:61-74.  Two forms over the same words:
 *
 * Host-driven, one merge per call (vocabularies above 4096, the host fallback on a string-hash
 * collision, the per-merge all-reduce form):
 * max over table[x][y], x,y < vcur, of (count << 32 | ~(x*Vt+y)) (0 if the table is empty)
 * into ws[2 + (call & 1)], where call = 0, 1, 2, ... numbers the calls on this workspace
 * (each call zeroes the other slot for the next one: no memset per call).  Incremental:
 * ws caches each row's best; a row is rescanned only when beast_bpe_apply_argmax changed it
 * -- any other table write needs a fresh zero-filled ws.
 * ws: beast_bpe_argmax_workspace_bytes(Vt), zero-filled once before call 0. */
size_t beast_bpe_argmax_workspace_bytes(int Vt);
int beast_bpe_argmax(const uint32_t* table, int Vt, int vcur, uint64_t* ws, int call, void* stream);
/* Merge (a,b)->new_id in every word, left to right, non-overlapping (HF Word::merge);
 * HF's pair-count changes, per word times wcount (NULL = 1):
 * [0]: (x,a)  [1]: (x,new)  [2]: (b,y)  [3]: (new,y).
 * are accumulated into deltas[4][Vt] int32 (multi-GPU: all-reduce them, then
 * beast_bpe_apply_argmax).  sig: beast_bpe_word_signatures.  pair_count: the pair's count from
 * beast_bpe_argmax (a hint choosing LDS-privatised or direct delta atomics). */
int beast_bpe_merge(uint16_t* sym, const uint32_t* wstart, uint32_t* wlen, const uint32_t* wcount,
                    int64_t n_words, int a, int b, int new_id, const uint32_t* tlen, int max_token_length,
                    int32_t* deltas, int Vt, uint64_t* sig, int64_t pair_count, void* stream);
/* The step after a merge, fused with the next argmax: table += deltas (deltas consumed are
 * zeroed), table[a][b] = 0 (merged pair retired), tlen[new_id] = tlen[a] + tlen[b]; then the
 * argmax of beast_bpe_argmax (same ws, next call index) over x, y < vcur (vcur counting new_id). */
int beast_bpe_apply_argmax(uint32_t* table, int32_t* deltas, int Vt, int vcur, int a, int b, int new_id,
                           uint32_t* tlen, uint64_t* ws, int call, void* stream);

/* Device-driven, batched (the default): merges are decided on the GPU, several per pass and
 * exactly HF's sequence -- each pass takes the table's top pairs in HF order while none chains
 * onto a taken one (its right symbol a taken left symbol, or its left a taken right), no taken
 * pair was a self-pair or re-used an id, and no taken row's next key ranks above it
 * (csrc/bpe_loop.hip, "batched merges", has the proof); stop rules: vocab_size reached, count below min_frequency, log full.
 * Ids of new strings come from a (64-bit string hash, byte length) table of the vocabulary
 * (HF's id reuse); the host replays the log against the real strings.
 * tok_hash / tok_pow: per initial token, h = sum bytes[i] * P^(n-1-i) and P^n (mod 2^64) of its
 * UTF-8 string; tlen its length in HF units (characters of the byte-level string), max_tlen
 * the largest.  beast_bpe_loop_state returns device pointers to the state {int32 active, vcur,
 * n_merges, ...} and the log [max_merges][4] int32 {a, b, nid, reused} for the host to read. */
size_t beast_bpe_loop_workspace_bytes(int Vt, int max_merges);
int beast_bpe_loop_init(void* ws, size_t ws_bytes, int Vt, int max_merges, int n_tokens, int vocab_size,
                        int min_frequency, const uint64_t* tok_hash, const uint64_t* tok_pow, const uint32_t* tlen,
                        int max_tlen, void* stream);
int beast_bpe_loop_state(const void* ws, int Vt, int max_merges, const void** state, const void** log);
/* n_steps passes of (merge the decided batch over every word, apply + rank + decide the next),
 * two launches each; passes after the loop stopped are no-ops.  max_batch (2, 4 or 8) caps a
 * pass.  argws: beast_bpe_argmax_workspace_bytes(Vt), zero-filled; batch_ws:
 * beast_bpe_batch_workspace_bytes(Vt).  flags: BEAST_BPE_BATCH_INIT ranks every row and decides
 * the first batch before the passes (first call after beast_bpe_loop_init); _NO_MERGE / _NO_APPLY
 * leave out one launch of each pass -- the sharded form: each rank holds a shard of the words,
 * its merge launch writes the pair-count changes into deltas [beast_bpe_batch_delta_count(Vt)]
 * int32 (zero-filled once) instead of the table, the caller all-reduces (SUM) them, and the apply
 * launch adds them to every rank's identical table (deltas NULL: one GPU, the changes go straight
 * into the table).  apps (nullable, accounting): apps[m] += the pair occurrences merge m
 * rewrote in the distinct words.  Vt <= 4096. */
#define BEAST_BPE_BATCH_INIT 1
#define BEAST_BPE_BATCH_NO_MERGE 2
#define BEAST_BPE_BATCH_NO_APPLY 4
/* The int32 words of the state (beast_bpe_loop_state) a host reads, of its first 16: the loop
 * still runs; the vocabulary size; the merges logged; the passes decided. */
#define BEAST_BPE_STATE_ACTIVE 0
#define BEAST_BPE_STATE_VCUR 1
#define BEAST_BPE_STATE_NMERGES 2
#define BEAST_BPE_STATE_PASSES 9
size_t beast_bpe_batch_workspace_bytes(int Vt);
size_t beast_bpe_batch_delta_count(int Vt);
int beast_bpe_loop_batch(void* ws, int Vt, int max_merges, int n_steps, int max_batch, int flags, uint16_t* sym,
                         const uint32_t* wstart, uint32_t* wlen, const uint32_t* wcount, int64_t n_words,
                         uint32_t* tlen, int max_token_length, uint64_t* sig, uint32_t* table, uint64_t* argws,
                         void* batch_ws, size_t batch_ws_bytes, int vocab_size, int32_t* deltas, uint32_t* apps,
                         void* stream);
/* One-call training (round 4; SURVEY.md §8b's beast_bpe_train): FIGBPE.fit_from_sequences
 * (beast/beast_bpe_trainer.py:76-98 -> :61-74, HF BpeTrainer(vocab_size, min_frequency,
 * special_tokens, initial_alphabet = chr(0 .. max - min), max_token_length).train_from_iterator
 * over the strings "".join(map(chr, seq - min))) on one GPU, the steps above in order: min /
 * max, presence, alphabet (special tokens, then byte-level chars and the initial alphabet by
 * code point), pretok count / scan / emit, dedup, repack, signatures, pair table, the batched
 * loop, the host replay of its log.  tokens / seq_off [n_seq + 1] / cls_lut [lut_n >= max - min
 * + 1] (beast_tokenizer_amd/pretok.py class_lut) are DEVICE pointers; special_tokens n_special
 * NUL-terminated UTF-8 strings (host).  Outputs (HOST): the token range, the vocabulary as UTF-8
 * strings in id order (out_vocab_bytes[out_vocab_off[i] .. out_vocab_off[i+1])), the merges as
 * id pairs out_merges[2m], [2m+1] (merge m's token is their concatenation, the next new id
 * unless the string already had one).  Capacities: max_vocab >= max(vocab_size, alphabet),
 * max_merges_out >= vocab_size - alphabet (checked up front), vocab_bytes_cap >= the strings'
 * bytes (known only after training).  When an output is too small the call returns
 * BEAST_E_WORKSPACE with the required sizes in *out_n_vocab, *out_n_merges and out_vocab_off[0]
 * (vocabulary bytes); retry with those.  Synchronises the stream.  Vt <= 4096 runs the batched
 * device loop; 4096 < Vt <= 32768 the host-driven one (beast_bpe_argmax / _merge / _apply_argmax,
 * one host read per merge), as does a rerun after a full merge log or a 64-bit string-hash
 * collision of the batched loop; BEAST_E_UNSUPPORTED above 32768 (the dense pair table).  One
 * GPU; beast_bpe_train_comm below is the multi-rank form. */
int beast_bpe_train(const int64_t* tokens, const int64_t* seq_off, int64_t n_seq, const uint8_t* cls_lut,
                    int64_t lut_n, int vocab_size, int min_frequency, int max_token_length,
                    const char* const* special_tokens, int n_special, int64_t* out_min_token,
                    int64_t* out_max_token, char* out_vocab_bytes, size_t vocab_bytes_cap, int64_t* out_vocab_off,
                    int max_vocab, int* out_n_vocab, int32_t* out_merges, int max_merges_out, int* out_n_merges,
                    void* stream);

/* ---- The library's own RCCL communicator (round 5; SURVEY.md §8b's beast_comm_init / destroy
 * and the comm argument of the training call), for a multi-GPU caller without torch.distributed.
 * RCCL is bound at run time (librccl.so.1; inside a torch process the copy torch mapped), so the
 * library loads without it; every entry point returns BEAST_E_UNSUPPORTED when it is absent.
 * One process per GPU: rank 0 makes an id (beast_comm_unique_id, beast_comm_id_bytes() bytes),
 * the caller hands it to every rank, each calls beast_comm_init_rank with its own device.
 * beast_comm_init is the single-process form (one handle per listed device, out[ndev]). */
typedef struct beast_comm beast_comm;
#define BEAST_DT_U8 0
#define BEAST_DT_I32 1
#define BEAST_DT_U32 2
#define BEAST_DT_I64 3
#define BEAST_DT_U64 4
#define BEAST_DT_F32 5
#define BEAST_DT_F64 6
#define BEAST_OP_SUM 0
#define BEAST_OP_MIN 1
#define BEAST_OP_MAX 2
size_t beast_comm_id_bytes(void);
int beast_comm_unique_id(void* id_out);
int beast_comm_init_rank(int world, int rank, const void* id, int device, beast_comm** out);
/* The single-process form's collectives (beast_comm_init with ndev > 1, one host thread driving
 * every handle) must be issued between beast_comm_group_start() and beast_comm_group_end(), as
 * ncclGroupStart / ncclGroupEnd require; otherwise drive each handle from its own host thread.
 * beast_bpe_train_comm issues collectives of its own: call it from one host thread per handle. */
int beast_comm_init(int ndev, const int* devs, beast_comm** out);
int beast_comm_group_start(void);
int beast_comm_group_end(void);
/* n virtual ranks on one device (SURVEY.md §4.3's "N virtual ranks on one device"; tests and
 * rehearsal on a one-GPU box): out[n] handles of a world of n, each driven by its own host thread.
 * Every collective synchronises the caller's stream and meets the other ranks in host memory
 * (rank-ordered reductions), so the library's multi-rank code paths run where RCCL cannot form a
 * world > 1.  A rank that does not arrive within 120 s fails the collective on every rank. */
int beast_comm_init_virtual(int n, int device, beast_comm** out);
int beast_comm_destroy(beast_comm* comm);
int beast_comm_info(const beast_comm* comm, int* world, int* rank, int* device);
/* §8e's reductions on device buffers (in place when send == recv), stream-ordered: the running
 * bounds (MIN / MAX over [D*N] f32, beast/beast_bspline_tokenizer.py:362-389), the quantile
 * histograms and BPE pair tables (SUM). */
int beast_comm_allreduce(beast_comm* comm, const void* send, void* recv, int64_t count, int dtype, int op,
                         void* stream);
int beast_comm_allgather(beast_comm* comm, const void* send, void* recv, int64_t count, int dtype, void* stream);
/* rank r's counts[r] elements at recv + displs[r] on every rank; counts / displs HOST [world],
 * equal on every rank */
int beast_comm_allgatherv(beast_comm* comm, const void* send, void* recv, const int64_t* counts,
                          const int64_t* displs, int dtype, void* stream);
/* beast_bpe_train over every rank's shard of the sequences (SURVEY.md §8b's comm argument;
 * FIGBPE.fit_from_sequences with process_group, beast/beast_bpe_trainer.py:61-98): the token
 * range is all-reduced (MIN / MAX), the code-point presence (MAX), each rank pre-tokenises and
 * deduplicates its shard, the distinct words x counts are all-gathered once (rank order) and
 * every rank runs the batched loop on the union -- bpe_train.py's replicated form, no per-pass
 * collective (replicate != 0).  replicate == 0 is the sharded form: every rank keeps its own
 * words, the pair table is SUM-reduced once and each pass's pair-count changes are SUM-reduced
 * between its merge and apply launches (the host-driven loop: each merge's), so the words of
 * no single GPU need to hold the corpus.  Every rank returns the same vocabulary and merges; a
 * shard may be empty (n_seq 0, or sequences without tokens), in either form.  All ranks must call it with the same options.  A failure
 * on one rank (an allocation, a launch, a shard over 2^32 symbols) is agreed over the communicator
 * before the next collective (the status all-reduced with MAX), so every rank returns an error
 * together: the failing rank its own, the others its code with a message naming the cause.
 * comm == NULL is beast_bpe_train. */
int beast_bpe_train_comm(const int64_t* tokens, const int64_t* seq_off, int64_t n_seq, const uint8_t* cls_lut,
                         int64_t lut_n, int vocab_size, int min_frequency, int max_token_length,
                         const char* const* special_tokens, int n_special, int64_t* out_min_token,
                         int64_t* out_max_token, char* out_vocab_bytes, size_t vocab_bytes_cap, int64_t* out_vocab_off,
                         int max_vocab, int* out_n_vocab, int32_t* out_merges, int max_merges_out, int* out_n_merges,
                         beast_comm* comm, int replicate, void* stream);
/* Distinct words (HF BpeTrainer trains on word -> count): every word of >= 2 symbols is
 * matched by content (hash tag + symbol-by-symbol compare, so collisions never merge
 * different words); out_* get one entry per distinct word (its first-seen copy in sym),
 * out_wcount its multiplicity, *out_n (device int64) the number of distinct words.
 * Output order is unspecified (training results do not depend on it).  Words of 0 or 1
 * symbols are dropped (they hold no pair). out_* sized n_words.
 * Workspace: beast_bpe_dedup_workspace_bytes(n) sizes the hash table for n / 4 distinct words
 * (trajectory corpora repeat their words; K5 is 13 % distinct, and the smaller table stays in the
 * 256 MB Infinity Cache).  With more distinct words than that table holds the call still returns
 * BEAST_OK but writes *out_n = -1 (the outputs are then undefined): retry with a larger workspace
 * (the in-tree callers multiply it by 4).  beast_bpe_dedup_workspace_bytes_safe(n) sizes a table
 * of >= 2 n slots, which can never fill: with it *out_n is always the distinct count. */
size_t beast_bpe_dedup_workspace_bytes(int64_t n_words);
size_t beast_bpe_dedup_workspace_bytes_safe(int64_t n_words);
int beast_bpe_dedup_words(const uint16_t* sym, const uint32_t* wstart, const uint32_t* wlen, int64_t n_words,
                          void* workspace, size_t ws_bytes, uint32_t* out_wstart, uint32_t* out_wlen,
                          uint32_t* out_wcount, int64_t* out_n, void* stream);
/* One-pass setup (round 5): beast_bpe_pretok_count / _emit and beast_bpe_dedup_words fused.
 * Every sequence is pre-tokenised (one wave each, as beast_bpe_pretok_emit) and its words of >= 2
 * byte symbols go straight into the distinct-word table, identified by their code points (a
 * match is confirmed against the first occurrence in `tok` itself); no per-occurrence symbol
 * array is written.  out_info (device int64[4]): distinct words, words, byte symbols, flags --
 * bit 0: the table filled up (retry with 4x the workspace), bit 1: a row the one-pass kernel does
 * not take (over 512 code points, a code point outside [0, 2^31), token offsets from 2^32): run
 * the two-pass functions above instead.  Workspace: beast_bpe_pretok_dedup_workspace_bytes(total
 * tokens; 28 bytes a table slot); it keeps the distinct-word list for beast_bpe_pretok_dedup_repack, which writes the
 * same outputs as beast_bpe_dedup_words + beast_bpe_repack_words (words of >= 2 symbols in
 * length order, their counts), byte symbols made from the code points (byte2id as pretok_emit).
 * repack_ws_bytes >= beast_bpe_repack_workspace_bytes(n_distinct) + 8 * (n_distinct + 1). */
size_t beast_bpe_pretok_dedup_workspace_bytes(int64_t n_tokens);
int beast_bpe_pretok_dedup(const int64_t* tok, const int64_t* seq_off, int64_t n_seq, int64_t min_tok,
                           const uint8_t* cls_lut, int64_t lut_n, void* workspace, size_t ws_bytes, int64_t* out_info,
                           void* stream);
int beast_bpe_pretok_dedup_repack(const int64_t* tok, int64_t min_tok, const uint16_t* byte2id, void* workspace,
                                  size_t ws_bytes, int64_t n_distinct, void* repack_ws, size_t repack_ws_bytes,
                                  uint16_t* out_sym, uint32_t* out_wstart, uint32_t* out_wlen, uint32_t* out_wcount,
                                  int64_t* out_nsym, void* stream);
/* Copy words into one symbol array ordered by length (min(L, 255) buckets, order inside a
 * bucket unspecified); each word starts at a multiple of 4 symbols (8 bytes) and owns its length
 * rounded up to 4 (the padding is zero): the layout the merge loops read and write in 8-byte
 * units.  out_sym capacity >= sum of round_up(wlen, 4); *out_nsym (device int64) = symbols of
 * the padded layout.  wcount may be NULL. */
size_t beast_bpe_repack_workspace_bytes(int64_t n_words);
int beast_bpe_repack_words(const uint16_t* sym, const uint32_t* wstart, const uint32_t* wlen, const uint32_t* wcount,
                           int64_t n_words, void* workspace, size_t ws_bytes, uint16_t* out_sym,
                           uint32_t* out_wstart, uint32_t* out_wlen, uint32_t* out_wcount, int64_t* out_nsym,
                           void* stream);
/* Keep the words that still have >= 2 symbols (order unspecified); *out_n device int64.
 * wcount may be NULL (count 1). */
int beast_bpe_compact_words(const uint32_t* wstart, const uint32_t* wlen, const uint32_t* wcount, int64_t n_words,
                            uint32_t* out_wstart, uint32_t* out_wlen, uint32_t* out_wcount, int64_t* out_n,
                            void* stream);

/* ------------------------------------------------------- §8f rank 1: BPE codec ---
 * Per-row BPE inference with a trained byte-level model, replacing
 * beast/beast_bspline_bpe_tokenizer.py:175-198 (_discrete_to_bpe: per row
 * tokenizer.encode("".join(map(chr, row - min)), add_special_tokens=False).ids) and
 * :200-247 (_bpe_to_discrete: tokenizer.decode(ids, skip_special_tokens=True), ord + min).
 * HF tokenizers semantics: AddedVocabulary split on special tokens (leftmost-longest),
 * ByteLevel pre-tokeniser, BPE::merge_word / Word::merge_all (rank, pos) min-heap,
 * ByteLevel decoder + String::from_utf8_lossy.
 *
 * Merge map: (a, b) -> (rank, new_id), open addressing in device memory; merges in rank
 * order (a pair listed twice keeps its last rank, as HF's HashMap collect). ids < 65536. */
int beast_bpe_mergemap_log2cap(int n_merges);
size_t beast_bpe_mergemap_bytes(int n_merges);
int beast_bpe_mergemap_build(const int32_t* merge_a, const int32_t* merge_b, const int32_t* merge_new,
                             int n_merges, void* map, size_t map_bytes, void* stream);
/* Encode rows tok[row_off[r] .. row_off[r+1]) (int64 bins).  Shifted code point
 * v = tok - min_tok; status[r]: 0 ok, 1 some v < 0, 2 some v > max_span (max_span >= 0),
 * 3 v > 0x10FFFF, 4 surrogate, 5 v >= lut_n (no class), 6 row longer than max_row_cps /
 * max_row_syms.  byte2id[256]: vocab id of each byte-level char, -1 if absent (dropped, or
 * unk_id (fused when fuse_unk) if the model has an unk token).  Special tokens:
 * spec_cps[n_spec][64] code points, spec_len, spec_id.  Output: out_ids[r][0 .. out_len[r])
 * (row stride out_stride >= max_row_syms).  LDS per row: beast_bpe_encode_lds_bytes (one row
 * must fit 160 KiB, else BEAST_E_UNSUPPORTED); a workgroup holds the merge map once (when it
 * fits beside a row) and as many rows as fit, up to 16. */
size_t beast_bpe_encode_lds_bytes(int max_row_cps, int max_row_syms);
int beast_bpe_encode_rows(const int64_t* tok, const int64_t* row_off, int64_t n_rows, int64_t min_tok,
                          int64_t max_span, const uint8_t* cls_lut, int64_t lut_n, const int32_t* byte2id,
                          const void* map, int n_merges, const int32_t* spec_cps, const int32_t* spec_len,
                          const int32_t* spec_id, int n_spec, int unk_id, int fuse_unk, int max_row_cps,
                          int max_row_syms, int32_t* out_ids, int64_t out_stride, int32_t* out_len,
                          int32_t* status, void* stream);
/* The same encode by words (round 4), one launch, no workspace: each workgroup pre-tokenises
 * its rows (up to 16), merges every distinct word among them once (exact dedup by code points in
 * LDS) and gathers each row's ids.  Bit-exact with beast_bpe_encode_rows for models whose merges
 * only combine tokens made by earlier merges -- every trained model; the caller checks and uses
 * beast_bpe_encode_rows otherwise, or when the model has special tokens.  status as above plus
 * 7 (ST_FALLBACK): the row holds a word of more than 64 byte symbols; the caller re-encodes such
 * rows with beast_bpe_encode_rows.
 * wordmap: the merges as a two-choice bucketed cuckoo table of 1 << wordmap_log2b buckets,
 * built on the host by beast_bpe_wordmap_build_host into a buffer of beast_bpe_wordmap_bytes
 * (HOST pointers; it returns the bucket count's log2) and copied to the device (its first
 * 16 << log2b bytes). */
int beast_bpe_wordmap_log2buckets(int n_merges);
size_t beast_bpe_wordmap_bytes(int n_merges);
int beast_bpe_wordmap_build_host(const int32_t* host_merge_a, const int32_t* host_merge_b,
                                 const int32_t* host_merge_new, int n_merges, void* host_out, size_t bytes,
                                 int* host_log2b_out);
int beast_bpe_encode_rows_words(const int64_t* tok, const int64_t* row_off, int64_t n_rows, int64_t min_tok,
                                int64_t max_span, const uint8_t* cls_lut, int64_t lut_n, const int32_t* byte2id,
                                const void* wordmap, int wordmap_log2b, int unk_id, int fuse_unk, int max_row_cps,
                                int max_row_syms, int32_t* out_ids, int64_t out_stride, int32_t* out_len,
                                int32_t* status, void* stream);
/* Decode rows ids[row_off[r] .. row_off[r+1]).  tok_off[n_vocab+1] / tok_bytes: each id's
 * ByteLevel-decoded bytes; tok_skip[id] = 1 for special tokens (skip_special_tokens) and
 * unassigned ids.  out[r][0 .. min(count, L)) = code point + min_tok; out_count[r] = code
 * points decoded (the caller checks == L); status[r] bit 0: the row holds unk_id, bit 1: it
 * holds an id < -1 (the caller's mark for a value that is not a u32).  Id -1 is skipped. */
int beast_bpe_decode_rows(const int32_t* ids, const int64_t* row_off, int64_t n_rows, const int32_t* tok_off,
                          const uint8_t* tok_bytes, const uint8_t* tok_skip, int n_vocab, int unk_id,
                          int64_t min_tok, int L, int64_t* out, int32_t* out_count, int32_t* status,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BEAST_HIP_H */
