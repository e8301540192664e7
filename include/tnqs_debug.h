/* tnqs_debug.h -- kernel-level test entry points of libtnqs_hip.so (used by tests/ only; not part of the drop-in
 * boundary).  Host pointers, column-major interleaved complex, synchronous. */
#ifndef TNQS_DEBUG_H
#define TNQS_DEBUG_H
#include <stdint.h>
#include "tnqs.h"
#ifdef __cplusplus
extern "C" {
#endif
/* one-sided Jacobi on A (m x n): on return A = U*Sigma (columns), V (n x n) with A_in = (U Sigma) V^dagger. dtype: 0 c64, 1 c128 */
int tnqs_dbg_jacobi(int dtype, int m, int n, void* A_inout, void* V_out, int* sweeps_out);
/* preconditioned theta SVD kernel (kernels_svd.hip theta_svd_pre_kernel) on one ComplexF32 factor A (m x n, 2 <= n <= 64, n <= nq <= m <= 128) of theta = A Q^T with Q
 * (nq x n complex128, orthonormal columns): on return A = U Sigma (columns, any order), V (nq x n ComplexF32) = right singular vectors of theta in the same column
 * order.  reps > 0: also the average duration (ms, HIP events) of a launch over `copies` device-resident copies */
int tnqs_dbg_theta_svd_pre(int m, int n, int nq, void* A_inout, const void* Q, void* V_out, int* sweeps_out, int copies, int reps, double* ms_out, double* phase_us_out /* 6 doubles or NULL: load, Gram, Cholesky + conversion, sweeps, U Sigma, V */,
                           int cap /* > 0: only the cap largest singular triplets are formed, the other columns of A leave as sigma_j e_0; Q == NULL: A is theta itself, V (n x n) = its right singular vectors */);
/* timing of the plain LDS-resident ComplexF32 Jacobi (no V) on `copies` copies of A (m x n): average launch duration and the sweeps it took */
int tnqs_dbg_time_jacobi_f32(int m, int n, const void* A, int copies, int reps, double* ms_out, int* sweeps_out);
/* Cholesky of a Hermitian positive definite n x n complex128 matrix (n <= 128): L lower with G = L L^dagger, W = (L^-1)^dagger; *fail = 1 when a
 * pivot fell to tau * max diagonal or below */
int tnqs_dbg_chol(int n, const void* G, void* L_out, void* W_out, int* fail_out, double tau);
/* out[(s',n),(a,b)] = sum_{(s,k)} in[(s,k),(a,b)] X[(s,k),(s',n)] with in element (s,a,k,b) at s + D*(a + PA*(k + K*b)) */
int tnqs_dbg_fiber_gemm(int dtype, int D, int PA, int K, int PB, int Do, int No, const void* in, const void* X, void* out,
                        double* norm2_out, int use_mfma);
/* out[i + KK*j] = sum_{(a,b)} X[i,(a,b)] conj(Y[j,(a,b)]), i,j = (s,k), KK = D*K; acc64: accumulate in double (out complex128) */
int tnqs_dbg_gram(int dtype, int D, int PA, int K, int PB, const void* X, const void* Y, void* out, int acc64, int use_mfma);
/* c64 only: out[i + K*j] = sum ( X x_r M )[i,.] conj(Y[j,.]) with D = 1 and r = the first row leg (chi_r = 32, d = 2) */
int tnqs_dbg_gram_fused(int PA, int K, int PB, const void* X, const void* Y, const void* M, void* out);
/* the gate path's fused gauge + f64 Gram kernels on one ComplexF32 site tensor [2, chi...] (column-major): out (complex128, KK x KK, KK = 2 chi_b)
   = G[i + KK j] = sum X'[i, fibers] conj(X'[j, fibers]), X' = X x_r M rounded to f32, r = the lowest leg that is not bleg; chi_b = chi_r = 32 or 16 */
int tnqs_dbg_gauge_gram(int z, const int* chi, int bleg, const void* X, const void* M, void* out);
/* c64 only: out[c,jx,mid,jy,hi] = sum in[c,ix,mid,iy,hi] Mx[ix,jx] My[iy,jy]; element at c + C0*(ix + 32*(mid + NMID*(iy + 32*hi))) */
int tnqs_dbg_pair(int C0, int NMID, int NHI, const void* in, const void* Mx, const void* My, void* out);
/* c64 only, site tensor [d][chi_0]..[chi_{z-1}] column-major: out = in x_lx Mx x_ly My (chi_lx = chi_ly = 32; leg 0 allowed) */
int tnqs_dbg_pair_legs(int d, int z, const int* chi, int lx, int ly, const void* in, const void* Mx, const void* My, void* out);
/* c64 only: out[b + 32*b'] = sum (X x_lx M)[.., b on leg ly, ..] conj(Y[.., b' on leg ly, ..]) */
int tnqs_dbg_pair_gram(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* M, void* out);
/* c64 only: both Grams of the plane (lx, ly) in one pass: out_y keeps ly (lx absorbed with Mx), out_x keeps lx (ly absorbed with My) */
int tnqs_dbg_pair_gram2(int d, int z, const int* chi, int lx, int ly, const void* X, const void* Y, const void* Mx, const void* My, void* out_y, void* out_x);
/* timing only: average launch duration (ms, HIP events) of a chi = 32 plane kernel over `nsites` device-resident tensors [2][32]^4;
 * which = 0 pair product on legs (lx, ly), 1 both-messages pair-Gram */
int tnqs_dbg_bench_plane(int which, int nsites, int lx, int ly, int reps, double* ms);
/* ---- entry points that reach exactly the kernels of ONE engine launch, with several items per launch set up as the engine sets them up.  ComplexF32
 * only; the items' arrays are passed one after the other.  A shape the named kernel does not take is refused with TNQS_ERR_UNSUPPORTED (no fall-back);
 * *route_out (may be NULL) says which kernel ran: */
#define TNQS_DBG_ROUTE_X3 1            /* bf16 x 3 matrix-core kernel (kernels_x3.hip: x3_rowgemm64_kernel, x3_gram64_kernel) */
#define TNQS_DBG_ROUTE_F32 2           /* f32 matrix-core kernel (mfma_rowgemm_kernel<KB, NB, D>, mfma_gram64_kernel) */
#define TNQS_DBG_ROUTE_F64 3           /* mfma_gram128_f64_kernel<false> */
#define TNQS_DBG_ROUTE_F64_SHARED 4    /* mfma_gram128_f64_kernel<true> (every item has D K = 128) */
#define TNQS_DBG_ROUTE_HALF_LINES 5    /* mfma_pair16_kernel (planes that contain leg 0) */
#define TNQS_DBG_ROUTE_WHOLE_LINES 6   /* mfma_pair16w_kernel */
#define TNQS_DBG_ROUTE_SMALL_SCALAR 7  /* bp_small_site_kernel<1024>, scalar form */
#define TNQS_DBG_ROUTE_SMALL_MFMA16 8  /* bp_small_site_kernel<1024>, matrix-core form (bp_small_site_mfma16) */
/* register-direct fiber GEMM (the chi = 32 gate epilogue: D = 2, K = 32; chi = 64 mode products / epilogue; chi = 32 mode products): item i is
 * out_i[(s',n),(a,b)] = sum_{(s,k)} in_i[(s,k),(a,b)] X_i[(s,k),(s',n)] with in_i element (s,a,k,b) at s + D*(a + PA[i]*(k + K*b)), X_i (D K) x (D No[i]),
 * out_i element (s',a,n,b) at s' + D*(a + PA[i]*(n + No[i]*b)); D in {1, 2}, K in {32, 64}, 1 <= No[i] <= K; PA[i] a multiple of 32, or a divisor of 32
 * with PB[i] a multiple of 32 / PA[i].  norm2_out[i] = the sum of item i's norm partials (|out_i|^2); tpw <= 0: the engine's tiles per workgroup */
int tnqs_dbg_rowgemm(int D, int K, int nitems, const int* PA, const int* PB, const int* No, const void* in, const void* X, void* out, double* norm2_out,
                     int tpw, int* route_out);
/* matrix-core Grams out_i[p + KK*q] = sum_{(a,b)} X_i[p,(a,b)] conj(Y_i[q,(a,b)]), p, q = (s,k), KK = D K, shape = (D, PA, K, PB) per item:
 * 32 < max KK <= 64: f32 accumulation, out complex64 (the BP message Gram); 64 < max KK <= 128: f64 accumulation, out complex128, Y must be NULL
 * (the gate-path Gram).  Y == NULL: Y_i = X_i.  nchunks <= 0: the engine's chunking, else at most nchunks chunks per item */
int tnqs_dbg_gram_mfma(int nitems, const int* shape, const void* X, const void* Y, void* out, int nchunks, int* route_out);
/* chi = 16 plane kernels on site tensors [d][chi_0]..[chi_{z[i]-1}] (chi: the items' dimensions one after the other), planes (lx[i], ly[i]) of two
 * 16-dimensional legs; M: (Mx, My) per item, 2 x 256 complex64, M[i + 16 j].  pair16: out_i = in_i x_lx Mx x_ly My (items of one launch must be of one
 * kind: route).  spw <= 0: the engine's slices per workgroup, else a multiple of 4 */
int tnqs_dbg_pair16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int* route_out);
/* out_y[i] (16 x 16, b + 16 b') = sum (X_i x_lx Mx)[.. b on ly ..] conj(Y_i[.. b' on ly ..]); both[i] != 0: also out_x[i] = sum (X_i x_ly My)[.. d on lx ..]
 * conj(Y_i[.. d' on lx ..]); both[i] == 0: the single-message form (My = NULL, no partial_x; out_x[i] untouched) */
int tnqs_dbg_pair_gram2x16(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const int* both, const void* X, const void* Y, const void* M,
                           void* out_y, void* out_x, int spw);
/* ---- the chi = 32 plane kernels as the engine launches them (engine_bp.cpp launch_products / launch_plane_grams, engine_batch.cpp run_chains): ONE launch over nitems
 * items of different geometry, planned by the engine's plan_* function and launched by its launch_* function.  ComplexF32 only.  Item i is a site tensor
 * [d][chi_0]..[chi_{z[i]-1}] (chi: the items' dimensions one after the other) with the plane (lx[i], ly[i]) of two 32-dimensional legs; the items' arrays are passed one
 * after the other and every sub-array starts at a multiple of 256 bytes on the device.  M: (Mx, My) per item, 2 x 1024 complex64, M[i + 32 j].  spw <= 0: the plan
 * function's own rule, else that many slices per workgroup (any positive value up to 65536).  A shape pair_geometry does not cover -- a plane leg that is not
 * 32-dimensional, lx == ly, a lower plane leg above 8 elements without a companion leg, a site that needs a fourth slice counter -- is refused with
 * TNQS_ERR_UNSUPPORTED and nothing is written.  Optional outputs (each may be NULL): *route_out = TNQS_DBG_ROUTE_X3 or TNQS_DBG_ROUTE_F32 (TNQS_NO_BF16X3=1), *spw_out =
 * the slices per workgroup the plan chose, wg_begin_out[i] / nwg_out[i] = item i's first workgroup and its workgroups (= its partials per message), *total_wgs_out.
 * in == NULL (pair32) / X == NULL (pair_gram32): HOST ONLY, these outputs alone are filled and no device is touched (tests/test_plane32_ref_cpu.py).
 * tnqs_dbg_pair32: plan_pair + launch_mfma_pair (x3_pair_kernel / mfma_pair_kernel): out_i = in_i x_lx Mx_i x_ly My_i.  out holds `guard` elements, item 0, `guard`
 * elements, item 1, ..., `guard` elements; it goes up as the caller filled it and comes back whole */
int tnqs_dbg_pair32(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, const void* in, const void* M, void* out, int spw, int guard,
                    int* route_out, int* spw_out, int* wg_begin_out, int* nwg_out, int* total_wgs_out);
/* one pair-Gram launch of one form (the engine launches doubles and singles separately), then launch_reduce<float, float> over every item's nwg[i] partials per message.
 * form 0, both messages: plan_pair_gram2 + launch_mfma_pair_gram2 (x3_pair_gram2_kernel<false> / mfma_pair_gram2_kernel); out_y[i] (1024 complex64, b + 32 b') =
 * sum (X_i x_lx Mx)[.. b on ly ..] conj(Y_i[.. b' on ly ..]), out_x[i] = sum (X_i x_ly My)[.. d on lx ..] conj(Y_i[.. d' on lx ..]).
 * form 1, one message, on the route launch_plane_grams takes: plan_x3_pair_gram1 + launch_x3_pair_gram1 (x3_pair_gram2_kernel<true>, My = partial_x = null), under
 * TNQS_NO_BF16X3=1 plan_pair_gram + launch_mfma_pair_gram (mfma_pair_gram_kernel); Mx alone is read, out_y alone is written, out_x (may be NULL) is not touched.
 * The partial arrays live in one device buffer laid out as guard band, item 0's partials, guard band, ..., guard band, filled with 0xff bytes (an f32 NaN) before the
 * launch: a partial nobody wrote makes the item's sum NaN, a touched band is an error return.  out_y / out_x: guard, item 0 (1024 complex64), guard, ..., guard, up as
 * filled and back whole */
int tnqs_dbg_pair_gram32(int d, int nitems, const int* z, const int* chi, const int* lx, const int* ly, int form, const void* X, const void* Y, const void* M,
                         void* out_y, void* out_x, int spw, int guard, int* route_out, int* spw_out, int* wg_begin_out, int* nwg_out, int* total_wgs_out);
/* the tall route of the ComplexF32 theta SVD (Cholesky-QR preprocessing, Jacobi on R, A J, polishing sweeps where the pivot collapsed) on nitems matrices
 * A_i (m[i] x n[i], 2 <= n <= 128, n <= m <= 512): A_i <- U Sigma (columns); chol_fail[i]: a Cholesky pivot was refused; polished[i]: the polishing sweeps
 * ran on the item; sweeps[i]: sweeps of the Jacobi on R (each output array may be NULL).  (m > 256 is where svd_batch sends a ComplexF32 theta of more than 256 rows whose
 * n x n triangle fits the LDS, e.g. 260 x 12: the tall_* kernels walk the rows in blocks and hold up to the 512 rows of a theta; the polishing launch is then jacobi_kernel<float, 8>) */
int tnqs_dbg_svd_tall(int nitems, const int* m, const int* n, void* A, int* chol_fail, int* polished, int* sweeps);
/* the whole BP message of a small site (kernels_bp.hip bp_small_site_kernel<1024>): ONE launch over nitems (site, outgoing leg) pairs, sized by the largest item as
 * the engine sizes it.  Item i is a site tensor [d[i]][chi_0]..[chi_{z[i]-1}] (column-major) with the outgoing leg jo[i]; chi, present: the items' legs one after
 * the other; psi: the items' tensors one after the other; M: one chi_k x chi_k matrix M[q + chi_k qo] per leg of every item, in leg order (the slot of leg jo
 * included: the kernel has to skip it), read only where present[leg] != 0 -- 0 hands the kernel a null pointer, i.e. the identity.  On the device every tensor and
 * matrix starts at a multiple of 256 bytes, like the engine's sub-buffers.  form: -1 the engine's rule (matrix-core form iff every leg is 16-dimensional and the
 * element count is a multiple of 256), 0 the scalar form, 1 the matrix-core form (refused where the rule does not allow it).  out, new_msg, old_msg: chi_jo^2 numbers
 * per item, out[b + chi_jo b'], the items one after the other.  new_msg == NULL: out_i = the raw message.  new_msg != NULL: the epilogue runs as well (m / sum(m)
 * when normalize != 0 and the sum is not exactly zero; diff_out[i] = message_diff against old_msg_i, the identity where has_old[i] == 0 or old_msg == NULL) --
 * inside the kernel in the matrix-core form, by msg_finalize_kernel<float> on the one partial in the scalar form -- and out is left as it was.  route_out (may be
 * NULL): TNQS_DBG_ROUTE_SMALL_* per item.  z > 8, a leg > 32 or more than 8192 elements: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_small_site(int nitems, const int* d, const int* z, const int* chi, const int* jo, const void* psi, const void* M, const int* present, int form,
                        const void* old_msg, const int* has_old, int normalize, void* out, void* new_msg, double* diff_out, int* route_out);
/* the BP message epilogue (kernels_bp.hip msg_finalize_kernel<T>; dtype 0 c64, 1 c128): ONE launch over nitems messages.  Item i: nchunks[i] partials of chi[i]^2
 * numbers laid out [chunk][element], the items one after the other; new_msg_i = their sum, divided by its element sum when normalize != 0 and that sum is not
 * exactly zero; diff_out[i] = message_diff(new_msg_i, old_msg_i) (the identity where has_old[i] == 0 or old_msg == NULL) */
int tnqs_dbg_msg_finalize(int dtype, int nitems, const int* chi, const int* nchunks, const void* partials, const void* old_msg, const int* has_old, int normalize,
                          void* new_msg, double* diff_out);
/* the BP sweep order bp_update uses when no edge_sequence is given, as (src[i] -> dst[i]) vertex indices; *n_out = its length (2 ne) */
int tnqs_dbg_default_sequence(tnqs_handle h, int* src, int* dst, int cap, int* n_out);
/* the same order from the graph alone (nv vertices, ne undirected edges esrc[e] - edst[e]) together with the dependency level bp_update runs every message in
 * (messages of one level are launched together; which value a message reads is decided by the positions).  HOST ONLY: no device is touched, so the scheduling
 * logic of the BP update -- linear forests, edge sets that close cycles on periodic lattices -- is testable without a GPU (tests/test_bp_schedule.py) */
int tnqs_dbg_default_sequence_graph(int nv, int ne, const int32_t* esrc, const int32_t* edst, int* src, int* dst, int* level, int cap, int* n_out);
/* the step schedule tnqs_apply_gates walks, from the graph and the gates' vertex lists alone (nverts[i] = 1 or 2 vertices of gate i, one list after the other in
 * verts): steps are batches (maximal runs of pairwise vertex-disjoint gates, in list order) and BP updates (in front of a gate on two vertices that touches a
 * vertex a gate has acted on since the last update, and once at the end; none when update_cache == 0 -- apply_gates.jl:64-95).  step_of_gate[i] = the step gate i
 * runs in; step_is_bp[k] = 1 where step k is an update (the first cap steps); *nsteps_out = the number of steps.  Arity and vertex range are checked
 * (TNQS_ERR_INVALID), adjacency is not.  HOST ONLY: no device is touched (tests/test_gate_schedule.py) */
int tnqs_dbg_gate_schedule(int nv, int ne, const int32_t* esrc, const int32_t* edst, int ngates, const int32_t* nverts, const int32_t* verts, int update_cache,
                           int* step_of_gate, int* step_is_bp, int cap, int* nsteps_out);
/* the launches of one fiber GEMM pass (out = in x_(s,leg) X) as the engine plans them, from the items' shapes alone (csrc/fiber_plan.cpp plan_fiber_pass).
 * use: 0 single-leg stage of a mode-product chain, 1 gate epilogue, 2 generic whatever the shape (one-site gate, second factorisation pass, region operator);
 * dtype 0 c64, 1 c128; use_mfma / use_chi64: the two switches (TNQS_NO_MFMA / TNQS_NO_CHI64 unset = 1); shape: (D, PA, K, PB, Do, No) per item.
 * launches_out (the first cap launches, in stream order), 10 ints each: route (0 generic tiled, 1 f32 matrix-core tiles, 2 register-direct, 3 f64 matrix cores),
 * D and K of a register-direct launch (else 0), fibers per tile TR, tiles per workgroup, KKmax, NNmax, workgroups, items, 1 = general form of the f64 kernel.
 * items_out, 7 ints per item in the caller's order: its launch, its first workgroup, its workgroups (= norm partials), TA, TB, nta, ntb.
 * A site too large for the generic kernel: TNQS_ERR_UNSUPPORTED.  HOST ONLY: no device is touched (tests/test_fiber_plan.py) */
int tnqs_dbg_fiber_plan(int use, int dtype, int use_mfma, int use_chi64, int nitems, const int* shape, int* launches_out, int cap, int* nlaunches_out, int* items_out);
/* ---- loop corrections (csrc/kernels_loop.hip; dtype 0 c64, 1 c128; column-major matrices, the items' matrices one after the other in every array) ----
 * loop_cgemm_kernel<T>, ONE launch: C_i (m[i] x n[i]) = A_i (m[i] x k[i]) op(B_i); opB = 0: B_i is k[i] x n[i]; opB = 1: B_i is n[i] x k[i], op = conjugate transpose.
 * C holds `guard` elements, then C_0, `guard` elements, C_1, ..., `guard` elements: the whole array goes to the device as the caller filled it and comes back,
 * so the caller sees that nothing outside the C_i was written. */
int tnqs_dbg_loop_cgemm(int dtype, int opB, int nitems, const int* m, const int* n, const int* k, const void* A, const void* B, void* C, int guard);
/* loop_antiproject_kernel<T>, ONE launch: T_i (nr[i] x nc[i], in place) <- T_i - f_i (b_i^T T_i), f_i, b_i of nr[i] elements, no conjugate */
int tnqs_dbg_loop_antiproject(int dtype, int nitems, const int* nr, const int* nc, void* T_inout, const void* f, const void* b);
/* loop_trace_kernel<T> + its tail: out[i] (complex128) = sum_ab X_i[a,b] Y_i[b,a], X_i p[i] x q[i], Y_i q[i] x p[i] */
int tnqs_dbg_loop_trace(int dtype, int nitems, const int* p, const int* q, const void* X, const void* Y, double* out_re_im);
/* loop_branch_gram_kernel<T>, ONE launch: item i has three legs of dimensions dims[3 i .. 3 i + 2] = (x_0, x_1, x_2) and a contraction length k[i];
 * A_i, B_i are (x_0 x_1 x_2) x k[i], rows i_0 + x_0 (i_1 + x_0 x_1 ... ) i.e. leg 0 fastest.  C_i[(l_p0, l_p0'), (l_p1, l_p1'), (l_p2, l_p2')] = sum_kk A_i[l, kk] conj(B_i[l', kk]),
 * every pair (ket, bra) interleaved with the ket index faster, the pairs in the order p = order[3 i .. 3 i + 2] (a permutation of 0, 1, 2; order = NULL: 0, 1, 2).
 * C holds guard bands as for tnqs_dbg_loop_cgemm. */
int tnqs_dbg_loop_branch_gram(int dtype, int nitems, const int* dims, const int* order, const int* k, const void* A, const void* B, void* C, int guard);
/* ---- the kernels that post-process a BP cache and prepare a gate's environments (dtype 0 c64 = T float, 1 c128 = T double; column-major n x n matrices).  ONE launch
 * over nitems items of different n, descriptors filled as the engine fills them; on the device every array of every item starts at a multiple of 256 bytes.  Input
 * arrays hold the items' matrices one after the other (a slot for every item, read only where its `present` flag is not 0 -- 0 hands the kernel a null pointer, i.e.
 * the identity).  Every OUTPUT array with a `guard` holds guard elements, item 0, guard elements, item 1, ..., guard elements: it goes to the device as the caller
 * filled it and comes back whole, so the caller sees that nothing outside the items was written.  n > 256: TNQS_ERR_UNSUPPORTED as in the engine, nothing is written ----
 * msg_rescale_kernel<T>: rescale_messages! of one edge per item; present[2 i], present[2 i + 1]: me_i, mer_i */
int tnqs_dbg_msg_rescale(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, void* me_out, void* mer_out, int guard);
/* edge_scalar_kernel<T>: out_re_im[2 i], [2 i + 1] = sum_ab me_i[a,b] mer_i[a,b]; the array goes up as filled and comes back */
int tnqs_dbg_edge_scalar(int dtype, int nitems, const int* chi, const void* me, const void* mer, const int* present, double* out_re_im);
/* env_prepare_kernel<T>: H_i = (M_i + M_i^dagger) / 2, V_i = identity, both complex128; present[i] */
int tnqs_dbg_env_prepare(int dtype, int nitems, const int* n, const void* msg, const int* present, void* H_out, void* V_out, int guard);
/* env_finish_kernel<T>: from the complex128 eigen factors (A_i = H_i V_i, V_i): msqrt_i = H^1/2 and proj_i = H^1/2 H^-1/2 over the eigenvalues kept under cutoff[i]
 * (type T); flags_out[2 i] = all kept, flags_out[2 i + 1] = a negative eigenvalue beyond the cutoff (the array goes up as filled and comes back) */
int tnqs_dbg_env_finish(int dtype, int nitems, const int* n, const void* A, const void* V, const double* cutoff, void* msqrt_out, void* proj_out, int* flags_out, int guard);
/* symg_build_kernel<T>: from the complex128 eigen factors of both messages of an edge: rx, ry = conj((M + reg)^1/2), irx, iry = conj((M + reg)^-1/2) (complex128) and
 * Ce = Ce0 = rx ry^T (type T); *flag_out = 1 when any regularised eigenvalue of any item is negative (one flag per launch, cleared first, as in the engine) */
int tnqs_dbg_symg_build(int dtype, int nitems, const int* n, const void* AX, const void* VX, const void* AY, const void* VY, double reg, void* rx, void* ry, void* irx, void* iry,
                        void* Ce, void* Ce0, int* flag_out, int guard);
/* symg_finish_kernel<T>: from U Sigma and V (type T, singular triplets as columns in any order) and irx, iry (complex128): S_i (n[i] doubles, descending; guard counts
 * doubles), Xs_i = irx U S^1/2, Xd_i = iry conj(V) S^1/2 (type T) */
int tnqs_dbg_symg_finish(int dtype, int nitems, const int* n, const void* USigma, const void* Vsvd, const void* irx, const void* iry, void* Xs, void* Xd, double* S, int guard);
/* diag_kernel<T>: out_i = diag(S_i) (S: chi[i] doubles per item) */
int tnqs_dbg_diag(int dtype, int nitems, const int* chi, const double* S, void* out, int guard);
/* cscale_kernel<T>: dst_i = src_i (re[i] + i im[i]), len[i] numbers per item (any length) */
int tnqs_dbg_cscale(int dtype, int nitems, const int* len, const void* src, const double* re, const double* im, void* dst, int guard);
/* ---- two-site reduced density matrices of bonds (csrc/kernels_rdm.hip, csrc/engine_rdm.cpp) ----
 * edge_rdm_kernel<P>, ONE launch over nitems bonds (ptype 0: P = float, 1: P = double): partial_u / partial_v hold the items' Gram partials one after the other, item i's
 * as nchunks_x[i] chunks of (d_x[i] chi[i])^2 complex numbers [chunk][(s + d a) + d chi (s' + d a')]; scale_u[i], scale_v[i]: the pending scale factors, 0 hands the kernel
 * a null pointer (no factor pending).  out (complex128): `guard` elements, item 0 ((du dv)^2 elements), `guard` elements, item 1, ..., `guard` elements -- it goes to the device
 * as the caller filled it and comes back whole.  An item the kernel's LDS does not hold: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_edge_rdm(int ptype /*0 float, 1 double*/, int nitems, const int* du, const int* dv, const int* chi,
                      const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                      const double* scale_u, const double* scale_v, void* out, int guard);
/* the same kernel with one partial type per end: edge_rdm_kernel<Pu, Pv> (tnqs_rdm_paths contracts a carried environment, double, with an end's Gram partial) */
int tnqs_dbg_edge_rdm_mixed(int ptype_u /*0 float, 1 double*/, int ptype_v, int nitems, const int* du, const int* dv, const int* chi,
                            const int* nchunks_u, const int* nchunks_v, const void* partial_u, const void* partial_v,
                            const double* scale_u, const double* scale_v, void* out, int guard);
/* path_apply_kernel<P, T>, ONE launch over nitems items: L_out_i = scale_i^2 L_in_i T_i with L_in_i the sum of nchunks_in[i] chunks of (d chi_a)^2 numbers of type P
 * [chunk][(s + d a) + d chi_a (s' + d a')], T_i a chi_b^2 x chi_a^2 matrix of the state's type T[(b + chi_b b') + chi_b^2 (a + chi_a a')]; items one after the other in
 * L_in and T; scale[i] = 0 hands the kernel a null pointer.  L_out (complex128) is laid out as guard, item 0 (ksplit[0] chunks of (d chi_b)^2 complex128), guard, item 1, ...,
 * guard; it goes up as the caller filled it and comes back whole.  ksplit[i] = 0 means "as plan_path_apply chooses" (size L_out by tnqs_dbg_path_apply_plan).
 * d[i]^2 > 16: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_path_apply(int ptype_in /*0 float, 1 double*/, int dtype /*0 c64, 1 c128*/, int nitems, const int* d, const int* chi_a, const int* chi_b,
                        const int* nchunks_in, const int* ksplit, const void* L_in, const void* T, const double* scale /*0: null*/, void* L_out, int guard);
/* plan_path_apply on a launch of nitems items (host only): ksplit_out[i] = the column ranges item i gets (ksplit[i] where that is > 0), nrb_out[i] its row blocks */
int tnqs_dbg_path_apply_plan(int nitems, const int* chi_a, const int* chi_b, const int* ksplit, int* ksplit_out, int* nrb_out);
/* tnqs_rdm_paths with the bound on a batch's workspace given explicitly (bytes, >= 1); *nbatches_out (may be NULL): the batches of paths it ran */
int tnqs_dbg_rdm_paths_ws(tnqs_handle h, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out,
                          int64_t workspace_bytes, int* nbatches_out);
/* tnqs_rdm_edges with the bound on a batch's chain workspace given explicitly (bytes, >= 1); *nbatches_out (may be NULL): the batches of ends it ran */
int tnqs_dbg_rdm_edges_ws(tnqs_handle h, int n_edges, const int32_t* eu, const int32_t* ev, double* out,
                          int64_t workspace_bytes, int* nbatches_out);
/* ---- bond entanglement spectra (csrc/kernels_spectrum.hip, csrc/engine_spectra.cpp) ----
 * stages A-D of tnqs_bond_spectra over nitems bonds of different chi in ONE launch per stage, set up and sized exactly as the engine does (env_prepare<T>, jacobi<double> with V,
 * bond_rho_kernel<T>, jacobi<double> on W, bond_spectrum_finish_kernel; each Jacobi stage: the LDS-resident kernel over the items whose f64 matrix with V fits, chi <= 70, the global-memory one over the rest).
 * m1 / m2: the items' chi[i] x chi[i] messages u -> v / v -> u one after the other, column-major, in the dtype (0 c64, 1 c128); present[2 i] / present[2 i + 1] = 0 hands the
 * kernels a null pointer for m1 / m2 (the identity; the slot is not read).  The cutoff is 10 eps of the dtype's real type.  out (double): `guard` elements, item 0 (chi[0]
 * eigenvalues of rho / tr rho, descending), `guard` elements, item 1, ..., `guard` elements -- it goes up as the caller filled it and comes back whole; flags_out: one int per
 * item, bit 1: an eigenvalue of m2 at or below -cutoff, bit 2: tr rho not positive and finite.  chi > 256: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_bond_spectrum(int dtype, int nitems, const int* chi, const void* m1, const void* m2, const int* present, double* out, int* flags_out, int guard);
/* the pending real scale factor of the site tensor of v (a normalising gate only records 1/||psi_v||; the tensor the reference holds is the stored one times it): 1 when none is pending */
int tnqs_dbg_pending_scale(tnqs_handle h, int v, double* factor);
/* ---- the gate path's per-gate small algebra (csrc/kernels_theta.hip and the small_svd_* kernels of csrc/kernels_svd.hip; dtype 0 c64 = T float, 1 c128 = T double).  ONE launch
 * of every kernel over nitems gates / sites of different sizes; the descriptors are filled by the rules of engine_gates.cpp (gate_items, run_theta, second_pass, add_small_svd)
 * and the same launches run in the same order.  Inputs hold the items' arrays one after the other; on the device every sub-array starts at a multiple of 256 bytes.  Every
 * output array with a `guard` holds guard elements, item 0, guard elements, item 1, ..., guard elements (elements of the array's own type), goes up as the caller filled it and
 * comes back whole.  The small integer outputs (info, texp, failure flags, ranks) and truncerr are contiguous per launch as in the engine's read-back buffer: they go up as
 * filled and come back.  A gate with d^2 chi > 512 (or a site the named kernel does not take): TNQS_ERR_UNSUPPORTED as in the engine, nothing is written ----
 * HOST ONLY (no device is touched): the gate (d1 d2 x d1 d2 complex128, column-major, first vertex most significant) as an operator sum g = sum_k a_k (x) b_k, as gate_items()
 * gets it: *kappa_out terms, fa_out[k][s' + d1 s] (room for min(d1, d2)^2 d1^2 numbers), fb_out[k][s' + d2 s] (min(d1, d2)^2 d2^2) */
int tnqs_dbg_operator_sum(const void* gate, int d1, int d2, int* kappa_out, void* fa_out, void* fb_out);
/* the launches of run_theta(): gate_theta -> gate_theta_mm -> lowrank_g -> chol / chol_packed -> lowrank_m (ComplexF64: -> lowrank_bw -> lowrank_g -> chol -> lowrank_ll ->
 * lowrank_m) -> theta_scale.  Per item: dims = (d1, d2, chi); n_s = d_s chi; mode[2], rk[2], tau[2] per site: mode 0 eigen (GA = G V, GV = V, GW = V), 1 Cholesky (GV = L,
 * GW = (L^-1)^dagger), 2 explicit factor (GV = R^dagger, GW = R^+, rk columns); F1, F2: (GA, GV, GW) of site 1 / 2, three n_s x n_s complex128 matrices per item; gate as above;
 * maxdim (<= 0: none); lowrank_on: the operator-sum / low-rank switch (TNQS_NO_LOWRANK unset = 1).  stop_after: 0 gate_theta, 1 gate_theta_mm, 2 the low-rank block, 3 theta_scale.
 * low_sizes_out, 6 ints per item: the element counts of lowA (Mr K), lowB (Nc K), lowG, lowL (K K), lowQ (Nc K), lowL2c (2 K K: L2, then Lc = L1 L2; ComplexF64) -- 0 where the host
 * rule of gate_items() does not hand the workspace out (Mr = d1^2 chi, Nc = d2^2 chi, K = kappa chi).  info == NULL: only low_sizes_out is filled (HOST ONLY) and the call returns.
 * Outputs: info (8 ints per item), lam1 / lam2 (n_s doubles), idx1 / idx2 (n_s ints), theta, theta0 (Mr Nc numbers of T), thetaV (max(Mr, Nc)^2 numbers of T), lowA .. lowL2c
 * (complex128, sized by low_sizes_out), texp (1 int per item), lowfail (2 ints per item: the gate's failure flag -- pass 1, with pass 2 folded in by lowrank_ll -- and the raw flag of pass 2, which means nothing
 * where info[7] = 0: its Cholesky then ran on a Gram matrix nothing wrote) */
int tnqs_dbg_gate_theta(int dtype, int nitems, const int* dims, const int* mode, const int* rk, const void* F1, const void* F2, const double* tau, const void* gate,
                        const int* maxdim, int lowrank_on, int stop_after, int* low_sizes_out, int* info, double* lam1, double* lam2, int* idx1, int* idx2,
                        void* theta, void* theta0, void* thetaV, void* lowA, void* lowB, void* lowG, void* lowL, void* lowQ, void* lowL2c, int* texp, int* lowfail, int guard);
/* gate_finish_kernel<T> alone on what the SVD stage leaves.  Per item: dims = (d1, d2, chi); info_in = (r1, r2, wide, K): info[0], [1], [5], [7]; texp; theta: the rotated columns
 * (max(Mr, Nc) x min(Mr, Nc) numbers of T with Mr = r1 d1, Nc = r2 d2; any column order); thetaV: min(Mr, Nc)^2 numbers of T; lam (n_s doubles), idx (n_s ints; the first r_s are
 * read) and GW (n_s x n_s complex128) of both sites; maxdim, cutoff, normalize, chi_cap.  Outputs: S (chi_cap doubles per item, guard counts doubles), info_out (chi', status),
 * truncerr (1 double per item), X1 (n_1 x d1 chi_cap numbers of T), X2 (n_2 x d2 chi_cap) */
int tnqs_dbg_gate_finish(int dtype, int nitems, const int* dims, const int* info_in, const int* texp, const void* theta, const void* thetaV, const double* lam1, const double* lam2,
                         const int* idx1, const int* idx2, const void* GW1, const void* GW2, const int* maxdim, const double* cutoff, const int* normalize, const int* chi_cap,
                         double* S, int* info_out, double* truncerr, void* X1, void* X2, int guard);
/* the SVD stage between the two (csrc/gate_svd.cpp launch_theta_svd_stage, the function TwoSiteBatch::svd_and_finish calls): the gates' JacobiItems, svd_batch (theta_svd_pre_kernel,
 * jacobi_lds_kernel, jacobi_kernel, the tall route), then the recovery of V -- ONE call over nitems gates.  dyn = 0: the static regime, the kernels get the dimensions from the host
 * and nothing is offered to theta_svd_pre_kernel; dyn = 1: the run-ahead regime, the kernels read `info` on the device, every launch is sized from the bounds and the ComplexF32 gates
 * are offered to theta_svd_pre_kernel by the engine's rules -- refused with TNQS_ERR_UNSUPPORTED where a bound fails the engine's one_trip rule (theta within the LDS-resident
 * Jacobi, at most 256 rows).  Per item: dims = (d1, d2, n1, n2) with the bounds n_s = d_s chi (n_s d_s > 512: TNQS_ERR_UNSUPPORTED); info: 8 ints, uploaded as given, of which
 * (r1, r2) = info[0], [1] with 1 <= r_s <= n_s and info[7] = the columns of the low-rank factor alive on the device (0: none) are read -- the SVD runs on the m x ncol matrix with
 * m = max(r1 d1, r2 d2), nfull = min(r1 d1, r2 d2), ncol = info[7] or nfull (a wide theta is stored as its adjoint); K: the columns the host expects of the low-rank route (0: none);
 * has_q / Q: the gate has the orthonormal factor Q of theta = M Q^T -- Q holds, for the items with has_q only, n2 d2 K complex128 numbers each, the (r2 d2) x K matrix at their start;
 * rank_bounds: the rank each site CAN have (two per item; times d_s they decide the offer of theta as it stands); cap: the bond dimension cap (0: none).  recover_form: 0 the engine's
 * rule (ComplexF32: recover_v_mfma_kernel), 1 recover_v_kernel<T, 8>.  theta (in: the m x ncol matrix, out: U Sigma), theta0 (the m x nfull theta; comes back as it went) and
 * thetaV (out: V, nfull x ncol) hold max(n1 d1, n2 d2) * min(n1 d1, n2 d2) numbers of T per item (thetaV: max(..)^2) -- sized from the BOUNDS, as the engine's workspaces are, the
 * matrix at the start of its slot with the leading dimension m (thetaV: nfull) -- laid out as guard, item 0, guard, ..., guard; they go up as filled and come back whole.
 * sweeps_out[i] (may be NULL): info[4] after the launches.  route_out[i] (may be NULL): which kernel factorises the item, decided on the host from the same item and predicates.
 * theta == NULL: only route_out is filled (HOST ONLY) */
#define TNQS_DBG_ROUTE_SVD_PRE_LOWRANK 10   /* theta_svd_pre_kernel<512> on the low-rank factor, V through Q */
#define TNQS_DBG_ROUTE_SVD_PRE_THETA 11     /* theta_svd_pre_kernel<512> on theta itself */
#define TNQS_DBG_ROUTE_SVD_LDS 12           /* jacobi_lds_kernel<T, RQ>, V recovered */
#define TNQS_DBG_ROUTE_SVD_GLOBAL 13        /* jacobi_kernel<T, 4 / 8>, V recovered */
#define TNQS_DBG_ROUTE_SVD_TALL 14          /* svd_tall (Cholesky-QR route, ComplexF32), V recovered */
int tnqs_dbg_theta_svd_stage(int dtype, int dyn, int nitems, const int* dims, const int* info, const int* K, const int* has_q, const void* Q, const int* rank_bounds, const int* cap,
                             int recover_form, void* theta, void* theta0, void* thetaV, int* sweeps_out, int* route_out, int guard);
/* the second factorisation pass: qr2_rinv_kernel (stage 0: X1 = R1^+ only; GV, A2, V2, tau, GVout, GWout, rk may be NULL), then qr2_compose_kernel (stage 1: both, X1 formed on the
 * device).  Per item n x n complex128 matrices: first-pass GW, GV, lam (n doubles), idx (n ints), r; the eigen pair (A2 = G2 V2, V2) of the second Gram matrix; tau.  Outputs X1,
 * GVout, GWout (n x n complex128) and rk.  n > 256: TNQS_ERR_UNSUPPORTED */
int tnqs_dbg_qr2(int stage, int nitems, const int* n, const void* GW, const void* GV, const double* lam, const int* idx, const int* r, const void* A2, const void* V2, const double* tau,
                 void* X1, void* GVout, void* GWout, int* rk, int guard);
/* small_svd_prepare_kernel<T> -> the f64 Jacobi -> small_svd_finish_kernel on site tensors [d][low][chi_b][hi] of type T (shape: 4 ints per item) with N = low hi < n = d chi_b <= 256
 * (else TNQS_ERR_UNSUPPORTED): GA, GV (n x n complex128): column j < N of GV = left singular vector u_j of M[(s,b), outer] = conj(psi), GA[:, j] = sigma_j^2 u_j; columns >= N zero */
int tnqs_dbg_small_svd(int dtype, int nitems, const int* shape, const void* src, void* GA, void* GV, int guard);
/* ---- overlap of two states (csrc/kernels_inner.hip, csrc/engine_inner.cpp; dtype 0 c64, 1 c128) ----
 * inner_gram_kernel<T> followed by inner_finalize_kernel<T> with normalize = 0 (the chunk sum), ONE launch each over nitems items set up as engine_inner.cpp sets them up.
 * shape: (PA, Ka, Kb, PB) per item; X: the items' [PA][Ka][PB] arrays one after the other, Y likewise with Kb (Y == NULL: Y = X, every item then needs Ka == Kb).
 * out_i[a + Ka b] = sum_{p, q} X_i[p, a, q] conj(Y_i[p, b, q]) in the element type, laid out as guard, item 0 (Ka Kb numbers), guard, item 1, ..., guard: it goes up as the
 * caller filled it and comes back whole; the partials are guarded on the device as well.  max_chunks <= 0: the engine's chunking, else at most that many chunks per item;
 * nchunks_out[i] (may be NULL): the chunks item i was summed from.  route_out (may be NULL): TNQS_DBG_ROUTE_INNER_MFMA.  A dimension outside 1..64: TNQS_ERR_UNSUPPORTED
 * (there is no scalar form), nothing is written */
#define TNQS_DBG_ROUTE_INNER_MFMA 9    /* inner_gram_kernel<T>: v_mfma_f32_16x16x4_f32 (c64) / v_mfma_f64_16x16x4_f64 (c128) */
int tnqs_dbg_inner_gram(int dtype, int nitems, const int* shape, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard, int* route_out);
/* inner_finalize_kernel<T>, ONE launch over nitems messages.  Item i: nchunks[i] partials of rows[i] cols[i] numbers of the element type laid out [chunk][a + rows b], the
 * items one after the other; new_msg_i = their f64 sum, divided by its element sum when normalize[i] != 0 and that sum is not exactly zero; diff_out[i] =
 * message_diff(new_msg_i, old_msg_i) (the rectangular delta where has_old[i] == 0 or old_msg == NULL); sum_out[2 i, 2 i + 1] = the raw element sum.  new_msg: guard, item 0,
 * guard, ..., guard as above.  rows or cols outside 1..64: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_inner_finalize(int dtype, int nitems, const int* rows, const int* cols, const int* nchunks, const void* partials, const void* old_msg, const int* has_old,
                            const int* normalize, void* new_msg, double* diff_out, double* sum_out, int guard);
/* inner_scalar_kernel<T>, ONE launch over nitems vertex / edge scalars of the form network.  Item i: m_i, mr_i of rows[i] x cols[i] numbers [a + rows b], the items one after the
 * other (a slot for every item, read only where present[2 i] / present[2 i + 1] != 0 -- 0 hands the kernel a null pointer, i.e. the rectangular delta); rawsum[2 i, 2 i + 1]
 * (has_rawsum[i] == 0: a null pointer); normalize[i]; scale_a[i], scale_b[i] (has_scale[2 i], [2 i + 1] == 0: a null pointer).  out_re_im[2 i, 2 i + 1] = sum_ab m_i[a, b] mr_i[a, b],
 * times rawsum_i where that is given, normalize[i] != 0 and it is not exactly zero, times the scale factors given.  out_re_im: guard, item 0 (one complex128), guard, ..., guard
 * (guard counts complex128).  rows or cols outside 1..64: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_inner_scalar(int dtype, int nitems, const int* rows, const int* cols, const void* m, const void* mr, const int* present, const double* rawsum, const int* has_rawsum,
                          const int* normalize, const double* scale_a, const double* scale_b, const int* has_scale, double* out_re_im, int guard);
/* ---- boundary MPS (csrc/kernels_bmps.hip), launched as csrc/engine_bmps.cpp launches them (dtype 0 c64, 1 c128) ----
 * bmps_contract_kernel<T> and, where an item is chunked, bmps_reduce_kernel<T>: ONE launch each over nitems items of different shape.  Item i: C[m, n] = sum_k A[m, k] B[k, n]
 * (B conjugated where conjB[i] != 0); m, n, k are groups of ngroup[3 i], [3 i + 1], [3 i + 2] legs (0 .. 4 each) with dimensions dims[12 i + 0 .. 3] (M legs), [+ 4 .. 7] (N
 * legs), [+ 8 .. 11] (K legs) and element strides strides[24 i + ..]: + 0 .. 3 the M legs in A, + 4 .. 7 the M legs in C, + 8 .. 11 the N legs in B, + 12 .. 15 the N legs in C,
 * + 16 .. 19 the K legs in A, + 20 .. 23 the K legs in B.  sizes[3 i ..]: the elements of item i's A, B and C arrays; A, B: the items' arrays one after the other; C: guard, item
 * 0, guard, item 1, ..., guard (guard elements each), up as the caller filled it and back whole -- elements of C that no (m, n) addresses keep what they held.  An index
 * that would fall outside its array is TNQS_ERR_INVALID before anything runs.  force_chunks <= 0: the engine's chunking, else that many chunks per item where the
 * contracted range has as many blocks (32 indices for c64, 16 for c128); nchunks_out[i] (may be NULL): the chunks of item i */
int tnqs_dbg_bmps_contract(int dtype, int nitems, const int32_t* ngroup, const int32_t* dims, const int64_t* strides, const int32_t* conjB, const int64_t* sizes,
                           const void* A, const void* B, void* C, int guard, int force_chunks, int32_t* nchunks_out);
/* bmps_qr_kernel<T>, ONE launch over nitems matrices: A_i = Q_i Y_i, m[i] x n[i], m >= n, 1 <= n <= 64 (else TNQS_ERR_UNSUPPORTED, nothing written).  row_major[i] == 0: A_i and
 * Q_i are column-major (the gauge step towards higher positions), != 0: element (r, c) at r n + c (the step towards lower positions).  A: the items one after the other; Q (m n
 * numbers per item) and Y (n n, column-major, upper triangular): guard, item 0, guard, ..., guard */
int tnqs_dbg_bmps_qr(int dtype, int nitems, const int32_t* m, const int32_t* n, const int32_t* row_major, const void* A, void* Q, void* Y, int guard);
/* ---- sampling (csrc/kernels_sample.hip), launched as csrc/engine_sample.cpp launches them ----
 * site_prob_partial_kernel<T> on one site tensor of n = d k elements (site index fastest) and T = the tensor with its messages absorbed: partial holds `guard` doubles, the raw
 * nblocks x 16 array (partial[16 b + s] = workgroup b's share of diag[s] = Re sum_l T[s, l] conj(psi[s, l]); slots s >= d are not written), `guard` doubles; it goes up as the
 * caller filled it and comes back whole.  nblocks == 0: the engine's plan_site_prob; *nblocks_out (may be NULL) = the workgroups used.  partial == NULL: only *nblocks_out is
 * filled (HOST ONLY) */
int tnqs_dbg_site_prob(int dtype, int n, int d, const void* tabs, const void* psi, int nblocks, double* partial, int guard, int* nblocks_out);
/* site_draw_kernel, one launch per item as the engine launches one per step.  Item i: partials_i (nblocks[i] x 16 doubles, the items one after the other), d[i], neg_tol[i], the
 * uniform uniform[i] or, where use_counter[i] != 0, the counter-based one of counter[3 i .. 3 i + 2] = (seed, sample, step) (the kernel then gets a null uniform); draw[i].
 * p_out: 16 doubles per item of which the kernel writes d[i]; x_out, px_out: one number per item (left as they were where draw[i] == 0); each laid out as guard, item 0, guard, ...,
 * guard (elements of its own type), up as filled and back whole.  status_out[i]: the item's own status word, cleared before its launch (1: tr rho zero / negative / not finite,
 * 2: a diagonal entry below -neg_tol tr) */
int tnqs_dbg_site_draw(int nitems, const int* nblocks, const int* d, const double* partials, const double* neg_tol, const double* uniform, const int* use_counter,
                       const uint64_t* counter, const int* draw, double* p_out, int* x_out, double* px_out, int* status_out, int guard);
/* site_project_kernel<T>: out[i] = psi[x + d i], i < nout (psi: nout d numbers); x_on_device != 0: x goes through device memory and the kernel's host argument is one that clamps
 * to another index; x outside 0 .. d - 1 is handed over as it is (the kernel clamps).  out: guard, nout numbers, guard */
int tnqs_dbg_site_project(int dtype, int nout, int d, const void* psi, int x, int x_on_device, void* out, int guard);
/* ---- the ComplexF32 d = 2 one-site gate with normalisation (csrc/kernels_util.hip: site1_c64_kernel, norm_factor_kernel, scale_kernel<T>) ----
 * ONE launch of site1_c64_kernel over nitems tensors of npairs[i] (s = 0, 1) pairs, the items one after the other in `in`; gates: per item the 2 x 2 gate as the C ABI takes it
 * (column-major G[s' + 2 s], 8 doubles re/im), packed into the kernel's item by the function the engine packs it with; nbx workgroups per item (the engine: 64).  out: guard, item 0,
 * guard, ..., guard (complex64).  normalize != 0: partials (guard doubles, nitems nbx norm partials [item][workgroup], guard doubles) are written and ONE launch of norm_factor_kernel
 * leaves factors (guard, 1 / sqrt(sum of item 0's partials), guard, ..., guard); normalize == 0: the kernel gets a null pointer and both arrays come back as they went up */
int tnqs_dbg_site1(int nitems, const int* npairs, const void* in, const double* gates, int nbx, int normalize, void* out, double* partials, double* factors, int guard);
/* norm_factor_kernel, ONE launch: factors_i = 1 / sqrt(sum of item i's npart[i] >= 0 partials), 1 where the sum is not positive; factors: guard, item 0 (one double), guard, ... */
int tnqs_dbg_norm_factor(int nitems, const int* npart, const double* partials, double* factors, int guard);
/* scale_kernel<T>, ONE launch: dst_i = src_i * (T)factor[i], len[i] numbers per item (any length); the factors are read from device memory as a pending scale factor is */
int tnqs_dbg_scale(int dtype, int nitems, const int* len, const void* src, const double* factor, void* dst, int guard);
/* tnqs_inner_bp with the bound on a batch's chain workspace given explicitly (bytes, >= 1); *nbatches_out (may be NULL): the batches of messages it ran */
int tnqs_dbg_inner_bp_ws(tnqs_handle ket, tnqs_handle bra, const tnqs_bp_opts* opts, double* out_log_re_im, int* niter, double* final_diff, int64_t workspace_bytes, int* nbatches_out);
/* ---- bitstring amplitudes (csrc/kernels_amp.hip, csrc/engine_amp.cpp; dtype 0 c64, 1 c128), launched as the engine launches them for one chunk of strings ----
 * amp_leg_gemm_kernel<T>, ONE launch over the groups of nitems jobs.  shape: (d, PA, K, PB, nstr) per job; T: the jobs' site tensors [d][PA][K][PB] one after the other;
 * x: nstr site values per job (0 .. d - 1), one after the other; M: the strings' message vectors [K][nstr] per job (has_m[i] == 0: the kernel gets a null pointer, all ones).
 * Per job and value g the strings with x = g form one item (group) whose index list is built as the engine builds it; a value no string takes gives no item.
 * R_i[(a + PA b') + PA PB p] = sum_k T_i[x_p + d (a + PA (k + K b'))] M_i[k + K p], laid out as guard, job 0 (PA PB nstr numbers), guard, ..., guard: it goes up as the
 * caller filled it and comes back whole.  K outside 1..64: TNQS_ERR_UNSUPPORTED (there is no scalar form), nothing is written */
int tnqs_dbg_amp_leg_gemm(int dtype, int nitems, const int* shape, const void* T, const int32_t* x, const void* M, const int* has_m, void* R, int guard);
/* amp_absorb_kernel<T>, ONE launch over nitems steps.  shape: (PA, K, PB, nstr) per step; in_i [PA][K][PB][nstr], m_i [K][nstr] (a slot for every step; has_m[i] == 0: a null
 * pointer, all ones); out_i[a + PA (b' + PB p)] = sum_k in_i[a, k, b', p] m_i[k, p], guarded as above.  K outside 1..64: TNQS_ERR_UNSUPPORTED, nothing is written */
int tnqs_dbg_amp_absorb(int dtype, int nitems, const int* shape, const void* in, const void* m, const int* has_m, void* out, int guard);
/* amp_finalize_kernel<T>, ONE launch over nitems messages of chi[i] numbers for nstr[i] strings: raw_i, old_msg_i [chi][nstr] (a slot for every item; has_old[i] == 0: a null
 * pointer, all ones); done (may be NULL): one int per string, the items one after the other.  Per string p: sum_out = the raw element sum (two doubles), new_msg = raw / sum
 * when normalize[i] != 0 and the sum is not exactly zero, diff_out = message_diff(new, old).  A string whose done flag is set: nothing of it is stored -- diff_out and sum_out
 * come back as they went up -- and its old message is carried over into new_msg bit for bit.  new_msg guarded as above.  chi outside 1..64: TNQS_ERR_UNSUPPORTED */
int tnqs_dbg_amp_finalize(int dtype, int nitems, const int* chi, const int* nstr, const void* raw, const void* old_msg, const int* has_old, const int* normalize, const int* done,
                          void* new_msg, double* diff_out, double* sum_out, int guard);
/* tnqs_amplitudes_bp with the workspace bound given explicitly (bytes, >= 1): it sizes the batches of jobs AND the chunks of strings; *nbatches_out (may be NULL): the
 * (batch of messages, chunk of strings) pairs it ran */
int tnqs_dbg_amplitudes_bp_ws(tnqs_handle h, int nstrings, const int32_t* configs, const tnqs_bp_opts* opts, double* out_log_re_im, int32_t* niter, double* final_diff,
                              int32_t* flags, int64_t workspace_bytes, int* nbatches_out);
/* ---- the ComplexF64 kernels of csrc/kernels_f64.hip as the engine launches them: ONE launch over items of different sizes.  The items' arrays are passed one after
 * the other; on the device every sub-array starts at a multiple of 256 bytes; each output with a `guard` is laid out as guard, item 0, guard, ..., guard (elements of
 * its own type), goes up as the caller filled it and comes back whole.  Nothing is refused for its shape: a launch the matrix-core kernel does not take runs on the
 * generic vector kernel, as in the engine, and *route_out says so */
#define TNQS_DBG_ROUTE_FIBER_GENERIC 15      /* fiber_gemm_kernel<double, 8> (generic vector kernel) */
#define TNQS_DBG_ROUTE_FIBER_F64_PLAIN 16    /* mfma_fiber_gemm_f64_kernel<NBLK, KS, false>: D = Do = 1, no norm partials */
#define TNQS_DBG_ROUTE_FIBER_F64_GENERAL 17  /* mfma_fiber_gemm_f64_kernel<NBLK, KS, true> */
#define TNQS_DBG_ROUTE_GRAM_GENERIC 18       /* gram_kernel<double, double, 4> (generic vector kernel) */
#define TNQS_DBG_ROUTE_GRAM_F64IN 19         /* mfma_gram_f64in_kernel */
/* ONE ComplexF64 fiber pass planned by plan_fiber_pass(items, nitems, fiber_rules(use, f32 = false, use_mfma, true), 16) and launched through launch_fiber_route<double>,
 * as FiberPass::launch<double> launches it.  use: 0 single-leg stage of a mode-product chain (every item needs D = Do = 1 and want_norm = 0, as the engine's have), 1 gate
 * epilogue.  shape: (D, PA, K, PB, Do, No) per item, item i as in tnqs_dbg_rowgemm: in_i (D K) x fibers, X_i (D K) x (Do No), out_i (Do No) x fibers, complex128.
 * tpw > 0 sets the tiles per workgroup of the f64 kernel (FiberRules::f64_tpw), tpw <= 0 takes the rule's value.  partials: guard doubles, one double per workgroup of
 * the launch, guard doubles; item i's norm is the sum of its slots wg_begin_out[i] .. wg_begin_out[i] + nwg_out[i] - 1, written only where want_norm[i] != 0 (the chain
 * launch is handed the array as well, so that a write shows).  inst_out: (NBLK, KS, GEN) of the instantiation launched, zeros on the generic route.  route_out, inst_out,
 * wg_begin_out, nwg_out may be NULL.  in == NULL: only these four are filled (HOST ONLY, no device is touched) */
int tnqs_dbg_fiber_pass_c128(int use, int use_mfma, int nitems, const int* shape, const int* want_norm, const void* in, const void* X, void* out, double* partials, int tpw,
                             int guard, int* route_out, int* inst_out, int* wg_begin_out, int* nwg_out);
/* ONE ComplexF64 Gram launch (launch_gram_route<double, double>) followed by launch_reduce<double, double> over all items; route (gram_route), tiles and chunks set up as
 * run_grams<double, double> sets them up.  shape: (D, PA, K, PB) per item; same[i] != 0: Y_i = X_i with the same device pointer (the item's slot in Y is not read; Y may be
 * NULL when every item is `same`).  out_i[p + KK q] = sum_{(a,b)} X_i[p,(a,b)] conj(Y_i[q,(a,b)]), KK = D K, complex128, guarded.  The partials are guarded on the device as
 * well; a touched guard there is an error return.  max_chunks <= 0: the engine's chunking, else at most that many chunks per item; nchunks_out[i] (may be NULL): the chunks
 * item i was summed from.  route_out (may be NULL): TNQS_DBG_ROUTE_GRAM_F64IN or TNQS_DBG_ROUTE_GRAM_GENERIC.  X == NULL: only route_out and nchunks_out are filled (HOST ONLY) */
int tnqs_dbg_gram_c128(int use_mfma, int nitems, const int* shape, const int* same, const void* X, const void* Y, void* out, int max_chunks, int* nchunks_out, int guard,
                       int* route_out);
/* the Gram route rule itself (csrc/kernels.hip gram_route, the function run_grams, tnqs_dbg_gram and tnqs_dbg_gram_c128 ask), from values alone: dtype 0 c64, 1 c128; acc64:
 * accumulation in double; has_m: the jobs carry a matrix to absorb; all_same: X == Y on every job; all_f64in: every job has 4 <= D K <= 64 and carries no matrix; the two
 * switches.  *route_out: 0 generic, 1 Mfma32, 2 Mfma64, 3 Fused32, 4 F64x64, 5 F64x128, 6 F64In, 7 Gauge64, 8 Gauge32 (the order of GramRoute).  HOST ONLY */
int tnqs_dbg_gram_route(int dtype, int acc64, int has_m, int all_same, int all_f64in, int kkmax, int use_mfma, int use_chi64, int* route_out);
/* ---- the small kernels that otherwise run inside larger calls only (csrc/debug_misc.cpp): each entry point calls the engine's own launch_* / plan_* function.  dtype 0 c64,
 * 1 c128; on the device every sub-array starts at a multiple of 256 bytes; an output with a guard is laid out as guard, item 0, guard, ..., guard, goes up as the caller
 * filled it and comes back whole ----
 * permute_kernel<T> (launch_permute): out[e] = in[sum_k idx_k stride_in[k]] with e = idx_0 + dims_out[0] (idx_1 + ...), 1 <= ndim <= 8.  A source index outside
 * 0 .. in_elems - 1 is TNQS_ERR_INVALID before anything runs.  guard in elements */
int tnqs_dbg_permute(int dtype, int ndim, const int32_t* dims_out, const int64_t* stride_in, int64_t in_elems, const void* in, void* out, int guard);
/* random_fill_kernel<T> (launch_random_fill): n iid normal entries of standard deviation `scale` per part from `seed`; real_only: imaginary parts 0.  guard in elements */
int tnqs_dbg_random_fill(int dtype, int64_t n, uint64_t seed, double scale, int real_only, void* out, int guard);
/* identity_kernel<T> (launch_identity): the n x n identity.  guard in elements */
int tnqs_dbg_identity(int dtype, int n, void* out, int guard);
/* sum_doubles_kernel (launch_sum_doubles): *out = sum of in[0 .. n - 1], n >= 0 */
int tnqs_dbg_sum_doubles(int n, const double* in, double* out);
/* record_pack_kernel, ONE launch over nitems records, then header_gather_kernel over pointers to those records.  info: 4 ints per item; terr: one double per item; S: nS[i]
 * doubles per item, X2: x2_words[i] 8-byte words per item, both one item after the other (x2_words[i] == 0: the kernel gets a null pointer).  Record i (dst_bytes[i] bytes)
 * = (info[2], info[3], terr, 0) as doubles | S | ... | X2 at byte x2_off[i]; what lies between and behind the parts is not written.  dst: guard, record 0, guard, ...,
 * guard, the guard in BYTES.  headers_out: 4 doubles per item.  A record that does not hold its parts is TNQS_ERR_INVALID */
int tnqs_dbg_record_pack(int nitems, const int32_t* info, const double* terr, const double* S, const int32_t* nS, const void* X2, const int64_t* x2_words, const int64_t* x2_off,
                         const int64_t* dst_bytes, void* dst, double* headers_out, int guard);
/* copy_items_kernel (launch_copy_items), ONE launch: item i is n16[i] 16-byte words followed by tail8[i] (0 or 1; tail8 == NULL: none) 8-byte words.  guard in BYTES */
int tnqs_dbg_copy_items(int nitems, const int64_t* n16, const int32_t* tail8, const void* src, void* dst, int guard);
/* plan_loop_dot + launch_loop_dot<T> (loop_dot_kernel<T> and its tail), ONE launch: out_i = sum_e X_i[e] Y_i[e] (bilinear, no conjugate) as two doubles, n[i] >= 0 elements.
 * The partials live in a guarded device buffer prefilled with NaN bytes.  nwg_out[i] (may be NULL): the workgroups the plan gives item i.  X == NULL: only nwg_out is
 * filled (HOST ONLY, no device is touched) */
int tnqs_dbg_loop_dot(int dtype, int nitems, const int64_t* n, const void* X, const void* Y, double* out_re_im, int32_t* nwg_out);
/* bmps_norm_kernel<T> (launch_bmps_norm), ONE launch over nitems vectors of n[i] elements: norm_out[i] = ||src_i||_2 (has_norm[i] == 0: a null pointer, norm_out[i] comes
 * back as it went up); dst_i = src_i (conjugated when conj[i]) times 1 / norm when normalize[i] and the norm is not 0 (has_dst[i] == 0: a null pointer; the item keeps
 * its place in dst).  guard in elements */
int tnqs_dbg_bmps_norm(int dtype, int nitems, const int64_t* n, const void* src, const int32_t* normalize, const int32_t* conj, const int32_t* has_dst, const int32_t* has_norm,
                       void* dst, double* norm_out, int guard);
/* amp_sweep_end_kernel (launch_amp_sweep_end): diffs[t nstrings + n]; per string n that is not done: fdiff = (sum_t diffs[t]) / nseq, niter = iter,
 * done = 1 when tol >= 0 and fdiff <= tol.  The three arrays go up as filled and come back */
int tnqs_dbg_amp_sweep_end(int nseq, int nstrings, int iter, double tol, const double* diffs, int32_t* done_inout, int32_t* niter_inout, double* fdiff_inout);
/* amp_scalar_kernel<T> (launch_amp_scalar) over nv + ne items in the engine's order (vertices, then edges): per string the sum over vertex items minus the sum over edge
 * items of log(sum_j m[j] mr[j]), as (log|.|, phase in (-pi, pi]); flags 1 an exactly zero item, 2 a non-finite one.  Every array holds a part for every item, one item
 * after the other: m, mr [chi[i]][nstrings] (present[2 i], present[2 i + 1] == 0: a null pointer, all ones); rawsum 2 nstrings doubles (has_rawsum[i] == 0: null; with
 * normalize[i] the item is multiplied by its string's rawsum unless that is exactly zero); scale one double (has_scale[i] == 0: null); site site_d[i] numbers (may be 0).
 * is_site[i] (vertex items only) makes item i an isolated vertex: its value is site_i[cfg[n ld + i]].  out_re_im (2 nstrings doubles) and flags_out are guarded, the
 * guard in their own elements.  chi outside 1..64: TNQS_ERR_UNSUPPORTED */
int tnqs_dbg_amp_scalar(int dtype, int nv, int ne, const int32_t* chi, const void* m, const void* mr, const int32_t* present, const double* rawsum, const int32_t* has_rawsum,
                        const int32_t* normalize, const double* scale, const int32_t* has_scale, const void* site, const int32_t* site_d, const int32_t* is_site,
                        const int32_t* cfg, int ld, int nstrings, double* out_re_im, int32_t* flags_out, int guard);
#ifdef __cplusplus
}
#endif
#endif
