/*
 * tnqs.h -- C ABI of libtnqs_hip.so: MI355X (gfx950) implementation of the BP-gauged
 * gate-application hot path of TensorNetworkQuantumSimulator.jl.
 *
 * The reference has no FFI seam (it is pure Julia); these entry points are what a
 * Julia shim type `HipBeliefPropagationCache <: AbstractBeliefPropagationCache` would `ccall`
 * (INTEGRATION.md shows the shim).  Each entry cites the reference function it replaces
 * (paths relative to the reference repository root).
 *
 * Conventions
 *   - every function returns an int status (0 = TNQS_OK, <0 = error); the message is available from
 *     tnqs_last_error() (thread-local).  No C++ exception crosses the ABI.
 *   - vertices are 0..nv-1, undirected edges are 0..ne-1 in the order given to tnqs_create; a directed
 *     edge is named by (src vertex, dst vertex).
 *   - host pointers are borrowed for the duration of the call only.
 *   - complex numbers are interleaved (re, im); matrices/tensors are column-major (Julia order).
 *   - canonical device layout of the site tensor of v:  [site d][leg to nbr_0]...[leg to nbr_{z-1}]
 *     column-major, neighbours in ascending vertex id.  Messages are chi x chi, index order (ket, bra).
 *   - one handle must not be used from two threads at once; every call is synchronous on return.
 */
#ifndef TNQS_H
#define TNQS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tnqs_state_s* tnqs_handle;

/* Element types (the reference's default is Float64, README.md:86; its BP tests run all four, test/test_beliefpropagation.jl:14,34).
 * A handle created as TNQS_F32 / TNQS_F64 takes and returns REAL site tensors and messages (tnqs_set/get_site_tensor,
 * tnqs_set/get_message); the device stores them as complex numbers with zero imaginary parts and runs the complex kernels.  Applying
 * a gate with a non-zero imaginary part promotes the handle to the complex type of the same precision, as in the reference
 * (`adapt_gate`, src/Apply/apply_gates.jl:41-44: a complex gate stays complex, and contracting it promotes the site tensors);
 * tnqs_scalartype tells which type the getters / setters currently speak. */
enum { TNQS_C64 = 0, TNQS_C128 = 1, TNQS_F32 = 2, TNQS_F64 = 3 };

enum {
    TNQS_OK = 0,
    TNQS_ERR_INVALID = -1,     /* bad argument; mirrors `error(...)` / ArgumentError in the reference */
    TNQS_ERR_UNSUPPORTED = -2,
    TNQS_ERR_HIP = -3,         /* HIP runtime failure (includes "no GPU") */
    TNQS_ERR_NUMERIC = -4,     /* e.g. sqrt of a negative message eigenvalue (Julia DomainError, src/utils.jl:21) */
    TNQS_ERR_COMM = -5
};

/* BP update options: kwargs of `update(bpc; maxiter, tolerance, edge_sequence, ...)`
 * (src/MessagePassing/abstractbeliefpropagationcache.jl:223-259, beliefpropagationcache.jl:51-72,103-117). */
typedef struct {
    int maxiter;          /* <= 0: reference default (25 on loopy graphs, 1 on trees) */
    double tolerance;     /* < 0: none (no convergence check) -- what `update(bpc; maxiter = 10)` means in the reference, whose
                           * default_tolerance(::Algorithm"bp") is `nothing`;  NaN: the tolerance of default_bp_update_kwargs
                           * (1e-5 f32 / c64, 1e-8 f64 / c128, none on trees), i.e. what apply_gates / truncate / normalize use when
                           * bp_update_kwargs is omitted.  A NULL opts pointer = default_bp_update_kwargs altogether */
    int normalize;        /* message_update_alg "contract" kwarg `normalize` (default true): m <- m / sum(m) */
    int n_sequence;       /* 0: library default edge sequence (linear forests -- on periodic lattices edge sets that close cycles --, DESIGN.md 4.3: the order the plane kernels share products on);
                           * -1: the reference's default, forest_cover_edge_sequence(graph) (beliefpropagationcache.jl:28), built by the library;
                           * > 0: the explicit sequence below */
    const int32_t* seq_src; /* explicit `edge_sequence` kwarg: directed edges, swept sequentially (Gauss-Seidel) */
    const int32_t* seq_dst;
} tnqs_bp_opts;

/* apply_kwargs of apply_gates / simple_update (src/Apply/simple_update.jl:21-24, forwarded to factorize_svd :58). */
typedef struct {
    int maxdim;             /* <= 0: no cap (`maxdim = nothing`) */
    double cutoff;          /* < 0: `cutoff = nothing` (behaves as 0: only exactly-zero weight is cut) */
    int normalize_tensors;  /* default true */
    double sqrt_cutoff;     /* < 0: default 10*eps(real(eltype)) (src/Apply/simple_update.jl:32-33) */
    int update_cache;       /* apply_gates kwarg `update_cache` (default true) */
} tnqs_apply_opts;

/* run statistics of the last tnqs_apply_gates / tnqs_truncate call (the reference only prints these when verbose) */
typedef struct {
    int n_bp_updates;       /* number of `update` calls triggered (c+1 for a TFIM layer) */
    int n_bp_sweeps;        /* total sweeps over all of them */
    int n_batches;          /* batched launches of pairwise-disjoint gates */
    int n_two_site;         /* two-site gates applied */
    int bp_not_converged;   /* updates that hit maxiter (reference: @warn, abstract...:245-252) */
    double last_bp_diff;
    int n_chol_fallbacks;   /* gate batches in which at least one site had a numerically rank-deficient Gram matrix (those sites take the eigen path) */
    int n_qr2_sites;        /* ComplexF64 sites that went through the second factorisation pass (ill-conditioned psi~) */
    int n_lowrank_svd;      /* two-site gates whose theta SVD ran on the low-rank factor (gate of operator Schmidt rank kappa, kappa chi < d chi) */
    int n_tall_svd;         /* theta SVDs that went through the Cholesky-QR preprocessing (matrix too tall for the LDS-resident Jacobi: 256 x 128 at chi = 64) */
    int n_svd_sweeps;       /* Jacobi sweeps of the theta SVDs, summed over the two-site gates of the call (diagnostic: sweeps per gate = this / n_two_site) */
    int n_svd_sweeps_max;   /* ... and the largest count of any single gate: a colour batch's SVD launch lasts as long as its slowest gate */
    int n_deferred_1site;   /* unitary one-site gates that were only recorded and later absorbed by a two-site gate on the vertex (or applied when the tensor was read) */
    int n_bp_products_reused;  /* BP: partial products (site tensor x messages of some legs) taken from an earlier level instead of recomputed */
    int n_bp_products_evicted; /* ... dropped again by the per-site bound (3) or the byte bound (TNQS_BP_CACHE_MB) before anything could reuse them or after */
    int n_lowrank_fallbacks; /* gates that qualified for the low-rank theta SVD but whose Cholesky / CholeskyQR2 of B refused a pivot: they took the SVD of the full theta */
    int n_spec_batches;     /* (library version 101) gate batches enqueued without their host round trip: every bond already at its cap, outcome verified afterwards */
    int n_spec_redone;      /* ... steps (gate batches, BP updates) whose deferred verification failed: state put back, step run again the careful way */
} tnqs_apply_stats;

/* ---- library ---------------------------------------------------------------------------------------- */
int tnqs_version(void);
const char* tnqs_last_error(void);
int tnqs_device_count(int* count);

/* ---- state handle: TensorNetworkState + BeliefPropagationCache(psi)
 *      (src/TensorNetworks/tensornetworkstate.jl:12-15, src/MessagePassing/beliefpropagationcache.jl:9-15,27-31).
 *      Created as the all-"up" product state with bond dimension 1 and unset (= identity) messages
 *      (tensornetworkstate.jl:72-75,141-161). */
int tnqs_create(int nv, int ne, const int32_t* edge_src, const int32_t* edge_dst, const int32_t* site_dim,
                int dtype, int device, tnqs_handle* out);
int tnqs_destroy(tnqs_handle h);
/* Base.copy(::BeliefPropagationCache) (beliefpropagationcache.jl:35-37): shallow, buffers are shared and
 * never mutated in place, so the copy is O(nv + ne). */
int tnqs_copy(tnqs_handle h, tnqs_handle* out);
/* scalartype(bpc) (abstractbeliefpropagationcache.jl:13): the element type host buffers of this handle are read / written in */
int tnqs_scalartype(tnqs_handle h, int* dtype);
/* use an existing HIP stream (e.g. torch's current stream) instead of the handle's own */
int tnqs_set_stream(tnqs_handle h, void* hip_stream);

/* ---- tensors / messages  (setindex_preserve! abstracttensornetwork.jl:40-43; psi[v]; setmessage!/message
 *      abstractbeliefpropagationcache.jl:93-102) ------------------------------------------------------------ */
/* leg_role[k] = -1 for the site leg, otherwise the neighbour vertex that leg k connects to.  The library
 * permutes into the canonical layout bit-exactly.  Bond dimensions of the incident edges are updated; messages
 * on an edge whose dimension changes are reset to the identity. */
int tnqs_set_site_tensor(tnqs_handle h, int v, const void* host, int ndim, const int64_t* dims, const int32_t* leg_role);
int tnqs_get_site_tensor(tnqs_handle h, int v, void* host, int ndim, const int32_t* leg_role);
/* Synthetic site tensor generated ON THE DEVICE (the benchmark states of the 8-GPU configurations are ~250 GiB: host random numbers plus PCIe
 * would take minutes): iid complex-normal entries (real-normal for a real handle), scaled by `scale`, in the canonical layout; bond_dims[j] =
 * dimension of the leg to the j-th neighbour in ascending vertex order.  Counter-based: entry e of vertex v depends on (seed, v, e) only, so
 * a sharded and an unsharded run build the same state.  Sharded handles: a vertex owned by another rank only records the dimensions. */
int tnqs_set_site_random(tnqs_handle h, int v, int n_neighbours, const int64_t* bond_dims, uint64_t seed, double scale);
int tnqs_site_tensor_size(tnqs_handle h, int v, int64_t* nelem);
/* chi x chi message src -> dst, axes (ket, bra), column major.  Every message the path itself produces is Hermitian to rounding, and tnqs_update absorbs some of them on
 * the bra side as their own conjugate transpose (csrc/engine_bp.cpp); a message handed in here that is NOT Hermitian (1e-5 / 1e-12 of its largest entry) makes the
 * handle (and its copies) absorb everything on the ket side, as abstractbeliefpropagationcache.jl:162-190 does. */
int tnqs_set_message(tnqs_handle h, int src, int dst, const void* host, int chi);
int tnqs_get_message(tnqs_handle h, int src, int dst, void* host, int chi);
int tnqs_bond_dim(tnqs_handle h, int u, int v, int* chi);           /* dim(virtualinds) */
int tnqs_maxvirtualdim(tnqs_handle h, int* chi);                     /* abstracttensornetwork.jl:27-29 */

/* ---- BP update (abstractbeliefpropagationcache.jl:223-259) -------------------------------------------------
 * Non-convergence is not an error (the reference only warns): status OK, *niter == maxiter, diff returned. */
int tnqs_bp_update(tnqs_handle h, const tnqs_bp_opts* opts, int* niter, double* final_diff);

/* ---- apply_gates (src/Apply/apply_gates.jl:46-98 incl. the update scheduling rule :68-90 and apply_gate!
 *      :101-143, simple_update src/Apply/simple_update.jl:21-77).  Mutates h (callers wanting the reference's
 *      value semantics call tnqs_copy first).
 *      gate_nverts[g] in {1,2}; gate_verts is the concatenation of the vertex lists; gate_mats is the
 *      concatenation of the d^k x d^k complex128 matrices, column-major, first listed vertex = most significant
 *      index.  out_truncerr is caller-allocated double[ngates] (apply_gates.jl:61). */
int tnqs_apply_gates(tnqs_handle h, int ngates, const int32_t* gate_nverts, const int32_t* gate_verts,
                     const double* gate_mats, const tnqs_apply_opts* opts, const tnqs_bp_opts* bp_opts,
                     double* out_truncerr, tnqs_apply_stats* stats);

/* ---- truncate (src/truncate.jl:12-38, edge_color = true branch).  Edge colour groups are supplied by the
 *      caller (the reference gets them from SimpleGraphAlgorithms.edge_color); n_groups = 0 selects the
 *      non-coloured branch (:31-35): one update after every edge in edge order. */
int tnqs_truncate(tnqs_handle h, int maxdim, double cutoff, int normalize_tensors, int n_groups,
                  const int32_t* group_offsets, const int32_t* edge_u, const int32_t* edge_v,
                  const tnqs_bp_opts* bp_opts, tnqs_apply_stats* stats);

/* ---- parity probes (src/expect.jl:59-82) ------------------------------------------------------------------
 * rho[s,s'] = sum psi[s,l..] conj psi[s',l'..] prod m[l,l'] (un-normalised, d x d complex128 col-major);
 * expect = tr(op rho)/tr(rho), op[s',s] column-major complex128. */
int tnqs_rdm_1site(tnqs_handle h, int v, double* out_rho);
int tnqs_expect_1site(tnqs_handle h, int v, const double* op, double* out_re_im);
/* Two-site reduced density matrices of bonds in one call (the reference's reduced_density_matrix(cache, [u, v]; alg = "bp") for adjacent u, v).  For request i = (u, v):
 *   rho[s_u, s_v ; s_u', s_v'] = sum_{a, a'} E_u[(s_u, a), (s_u', a')] E_v[(s_v, a), (s_v', a')],
 *   E_u[(s, a), (s', a')] = sum_rest (psi_u x_{k != v} m_{k -> u})[s, a, rest] conj(psi_u[s', a', rest]),
 * un-normalised (pending scale factors of the site tensors included, as in tnqs_rdm_1site), with the site dimensions the handle has NOW (1 for a projected vertex).
 * out_rho: the requests' (d_u d_v)^2 complex128 matrices one after the other, column-major, the FIRST listed vertex most significant (row = s_v + d_v s_u, column
 * likewise), so <O_u O_v> = tr(kron(O_u, O_v) rho) / tr(rho) with the gate convention above.  edge_u == NULL or edge_v == NULL: every edge in tnqs_create order as
 * (src, dst), n_edges is not read then; an empty call passes lists with n_edges = 0.  Both orientations and repeats are allowed: (v, u) returns the index-swapped matrix
 * of (u, v), a repeated request is answered again.  The handle is not changed apart from deferred one-site gates being applied first (as tnqs_rdm_1site does).
 * All ends of all distinct bonds are contracted in batches whose chain workspace stays under min(2 GiB, a quarter of the free device memory) -- a single end that needs
 * more runs alone -- and the call ends with one read-back.  ComplexF32 handles: ends with 8 <= d chi <= 64 accumulate in f32 inside a chunk on the matrix cores (the BP
 * message Gram's arithmetic), everything else (smaller, larger, or a bond whose other end is outside that range) in f64 on the generic kernel; chunks and the bond are
 * summed in f64.  TNQS_ERR_INVALID: a pair that is not an edge, a bad vertex; TNQS_ERR_UNSUPPORTED: sharded handles, (d_u^2 + d_v^2) chi beyond the bond kernel's LDS
 * (about 4096), d chi beyond the generic Gram kernel's. */
int tnqs_rdm_edges(tnqs_handle h, int n_edges, const int32_t* edge_u, const int32_t* edge_v, double* out_rho);
/* two-site density matrices of the ends of paths (reduced_density_matrix(cache, [u, w]; alg = "bp"), src/rdm.jl:52-73, with the path as the Steiner tree):
 * path q has path_len[q] >= 2 vertices, listed one after the other in path_verts; out_rho receives, for q = 0.., for k = 1 .. path_len[q]-1, the
 * un-normalised (d_p0 d_pk)^2 complex128 matrix of (p_0, p_k) in the layout of tnqs_rdm_edges */
/* With E as in tnqs_rdm_edges and T_k[(b, b'), (a, a')] the double-layer transfer matrix of the inner vertex p_k (messages of every leg off the path absorbed):
 *   L_0 = E_{p_0 -> p_1},  L_k[s, s'; b, b'] = sum_{a, a'} L_{k-1}[s, s'; a, a'] T_k[(b, b'), (a, a')],  rho_{p_0, p_k} = sum_{a, a'} L_{k-1}[s_u, s_u'; a, a'] E_{p_k -> p_{k-1}}[(s_w, a), (s_w', a')]
 * -- one path gives the matrix of (p_0, p_k) for every k; k = 1 is the bond's matrix of tnqs_rdm_edges.  L is complex128 with f64 accumulation from the first step on,
 * whatever the handle's type; it is NOT rescaled along the path (f64 range).  Paths must be INDUCED (no two non-consecutive vertices adjacent: the reference contracts the
 * induced region, so a chord is an argument error, not another answer; a shortest path is always induced).  Paths are taken in order in batches whose workspace stays under
 * min(2 GiB, a quarter of the free device memory) -- a path that needs more runs alone; ends and transfer matrices that several paths of a batch share are built once -- and
 * the call ends with one read-back.  The handle is not changed apart from deferred one-site gates being applied first.  npaths = 0 is a no-op.
 * TNQS_ERR_INVALID (before any device work): a bad vertex, consecutive vertices that are not adjacent, a repeated vertex, a chord, a length below 2, a null output;
 * TNQS_ERR_UNSUPPORTED: sharded handles, an inner vertex of degree above 7, chi_a^2 chi_b^2 above INT_MAX / 4, a bond beyond the edge kernel's LDS, d_p0 above 4. */
int tnqs_rdm_paths(tnqs_handle h, int npaths, const int32_t* path_len, const int32_t* path_verts, double* out_rho);
/* Entanglement spectra of bonds from the BP messages in one call (the reference's renyi_entropy(bp_cache, e; alpha), src/entanglement.jl:73-86, up to the eigenvalues).
 * For request i = (u, v) with m1 = message u -> v and m2 = message v -> u (layout of tnqs_get_message):
 *   r = m2^{1/2} from the Hermitian eigen decomposition of m2 in f64 whatever the handle's type, an eigenvalue x with |x| < cutoff replaced by 0, cutoff = 10 eps of the
 *   handle's real type (1.1920929e-6 / 2.220446e-15, absolute; pseudo_sqrt_inv_sqrt, src/utils.jl:18-26);  rho = r m1^T r;  spectrum = eigenvalues of rho / tr rho.
 * out_spectra: request i receives chi_i doubles (tnqs_bond_dim), one request after the other: descending, signed, summing to 1, UNFILTERED (the reference's renyi_entropy drops
 * |lambda| <= 10 eps before the logarithm; that is left to the caller).  edge_u == NULL or edge_v == NULL: every edge in tnqs_create order as (src, dst), n_edges is not read
 * then; an empty call passes lists with n_edges = 0.  Both orientations and repeats are allowed and each is computed as listed: the root is taken of the message TOWARDS the
 * first listed vertex ((u, v) and (v, u) have the same spectrum up to rounding).  All arithmetic is complex128 / f64 on the device from the stored messages, one workgroup per
 * request and one launch per stage over all requests of the call (workspace: 64 chi^2 bytes per request; each eigen stage is one launch of the LDS-resident Jacobi over the
 * bonds with chi <= 70 and one of the global-memory Jacobi over the rest); the call ends with one read-back.  The handle is not changed.
 * TNQS_ERR_INVALID (before any device work): a bad vertex, a pair that is not an edge, a null output with work to do; TNQS_ERR_UNSUPPORTED: sharded handles, chi > 256;
 * TNQS_ERR_NUMERIC: an eigenvalue of m2 at or below -cutoff (the reference's DomainError: square root of a negative real), or a trace of rho that is not positive and finite
 * (tnqs_last_error says which). */
int tnqs_bond_spectra(tnqs_handle h, int n_edges, const int32_t* edge_u, const int32_t* edge_v, double* out_spectra);
/* all-vertex <op_v>: ops is nv consecutive d x d matrices; out is nv complex128 */
int tnqs_expect_all(tnqs_handle h, const double* ops, double* out_re_im);

/* ---- multi-site observables (src/expect.jl:59-82) ------------------------------------------
 * The caller passes the region = the vertices of the Steiner tree of the observable's support (expect.jl:68), as a rooted
 * tree: region_parent[i] = index (into region_verts) of the parent of vertex i, -1 for the single root.  What is contracted is the
 * INDUCED region, as in the reference (norm_factors over the Steiner vertices share every internal bond): a bond between two region
 * vertices that is not a tree edge (a plaquette's closing bond) is summed over as well -- chi^2 tree contractions per such bond, at
 * most 2^16 terms in all (TNQS_ERR_UNSUPPORTED beyond: one closing bond up to chi = 256, two up to chi = 16).  ops = one d x d complex128 column-major matrix op[s',s] per region vertex
 * (identity off the support).  out = {Re, Im numerator, Re, Im denominator}; <O> = coeff * numer / denom. */
int tnqs_expect_region(tnqs_handle h, int n_region, const int32_t* region_verts, const int32_t* region_parent,
                       const double* ops, double* out_numer_denom);

/* ---- BP scalars and normalisation --------------------------------------------------------
 * vertex scalar  tr(rho_v)  = [psi_v, conj psi_v, incoming messages] contracted (abstractbeliefpropagationcache.jl:22-28),
 * edge scalar    sum_ij m_e[i,j] m_rev(e)[i,j]                                    (beliefpropagationcache.jl:47-49);
 * free energy = sum log(vertex scalars) - sum log(edge scalars) (abstract...:289-304) is left to the host.
 * out_vertex: nv complex128 (NaN for vertices owned by another rank); out_edge: ne complex128, edges in tnqs_create order.
 * tnqs_rescale: rescale_messages! then rescale_vertices! (beliefpropagationcache.jl:82-140, abstract...:318-322) in place:
 * afterwards every vertex and edge scalar is 1 (the BP norm of the state is 1). */
int tnqs_vertex_scalars(tnqs_handle h, double* out_vertex);
int tnqs_edge_scalars(tnqs_handle h, double* out_edge);
int tnqs_rescale(tnqs_handle h);
/* the two halves on their own, as the abstract cache interface has them (abstractbeliefpropagationcache.jl:11-20,306-316): generic callers
 * invoke either one.  tnqs_rescale_messages: rescale_messages!(bpc, edges) (beliefpropagationcache.jl:127-140) on the listed edges
 * (edge_u[i], edge_v[i]), both directions each; edge_u == NULL: every edge.  tnqs_rescale_vertices: rescale_vertices!(bpc, vertices)
 * (beliefpropagationcache.jl:82-101) with the vertex scalars under the CURRENT messages; vertices == NULL: every vertex. */
int tnqs_rescale_messages(tnqs_handle h, int n_edges, const int32_t* edge_u, const int32_t* edge_v);
int tnqs_rescale_vertices(tnqs_handle h, int n_vertices, const int32_t* vertices);

/* ---- symmetric (Vidal) gauge (src/symmetric_gauge.jl:1-62) ---------------------------------
 * per edge: psi_src <- psi_src X^-1/2 U S^1/2, psi_dst <- psi_dst Y^-1/2 V S^1/2 with U S V = svd(X^1/2 (Y^1/2)^T), X, Y the two
 * messages of the edge (eigenvalues + regularization before the roots); both messages := diag(S).  The state is unchanged and
 * diag(S) is a BP fixed point when the input messages were one.  regularization < 0: default 10 eps(real(eltype)). */
int tnqs_symmetric_gauge(tnqs_handle h, double regularization);

/* ---- sampling (src/sampling.jl:3-46, alg = "bp"; library version 102) ----------------------------------------------
 * psi_v <- psi_v[config, ...]: the site leg of v gets dimension 1 (setindex_preserve!(cache, psi_v * onehot(s => config)),
 * src/sampling.jl:35-36).  Bond dimensions and messages are kept; the tensor is not rescaled.  config in [0, d_v).  Afterwards
 * tnqs_set_site_tensor on v takes a site dimension of 1 and tnqs_apply_gates on v is TNQS_ERR_INVALID.  Sharded handles: TNQS_ERR_UNSUPPORTED. */
int tnqs_project_site(tnqs_handle h, int v, int config);
int tnqs_site_dim(tnqs_handle h, int v, int* d);                     /* the CURRENT site dimension (1 after tnqs_project_site) */
/* p[s] = real(diag rho_v)[s] / tr rho_v under the current messages, d_v doubles: the weights sample() draws from (src/sampling.jl:28-30),
 * from the same kernel tnqs_sample_bp uses.  TNQS_ERR_NUMERIC: tr rho_v zero or not finite, or a diagonal entry below
 * -(100 eps of the element's real type) tr rho_v (entries negative within that bound count as 0). */
int tnqs_site_probabilities(tnqs_handle h, int v, double* out_p);
/* sample(alg"bp") loop of src/sampling.jl:18-43 on COPIES of h (h is not changed; the caller has updated and, if wanted, gauged it): per
 * sample, at every vertex in vertex order: the weights above, a draw, tnqs_project_site, and (except after the last vertex) tnqs_bp_update
 * with bp_opts.  The draw takes ONE uniform u: x = the first s with u < p[0] + ... + p[s], the last s if there is none.
 * uniforms: NULL = the library's counter-based generator (the uniform of (seed, sample, vertex) depends on those three numbers only, 53 bits,
 * never 1); else nsamples*nv doubles in [0,1), sample-major.
 * out_config: nsamples*nv int32 in 0..d-1, sample-major, vertex order.  out_prob (may be NULL): the probability p[x] with which
 * each entry was drawn, same layout; log q(x) of a sample is the sum of their logs.  stats (may be NULL): BP updates / sweeps /
 * non-converged updates summed over the call.  For the same uniforms the result is exactly what the host loop over tnqs_copy,
 * tnqs_site_probabilities, that draw, tnqs_project_site and tnqs_bp_update gives.  Sharded handles: TNQS_ERR_UNSUPPORTED. */
int tnqs_sample_bp(tnqs_handle h, int nsamples, const tnqs_bp_opts* bp_opts, uint64_t seed, const double* uniforms,
                   int32_t* out_config, double* out_prob, tnqs_apply_stats* stats);

/* ---- loop corrections (src/MessagePassing/loopcorrection.jl:79-89 `weight`, for simple cycles) ------------------
 * Cycle c is the vertex list v_0 .. v_{L-1} (cycle_len[c] = L >= 3 distinct vertices, consecutive ones and the closing pair neighbours),
 * the lists one after the other in cycle_verts.  out_re_im[2c, 2c+1] = W(c) = Tr prod_k (A_k T_k): T_k the double-layer transfer matrix of
 * v_k on the bond pair (from v_{k-1}, to v_{k+1}) with the cache's messages on its other legs, A_k = I - vec(m_{v_k -> v_{k+1}})
 * vec(m_{v_{k+1} -> v_k})^T the antiprojector of the bond (bilinear, no conjugate).
 * PRECONDITION (not checked): the handle is rescaled (tnqs_rescale: every vertex and edge scalar is 1) -- only then is W the weight of the
 * loop series, Z = Z_bp (1 + sum W).  The handle is not changed.  ncycles = 0 is allowed.
 * Cycles are processed in batches whose workspace stays under min(2 GiB, a quarter of the free device memory); a single cycle that needs more than that is
 * still run on its own (its allocation may then fail with TNQS_ERR_HIP).
 * TNQS_ERR_INVALID: a list that is not a cycle of the graph; TNQS_ERR_UNSUPPORTED: sharded handles, vertex degree > 7. */
int tnqs_loop_weights(tnqs_handle h, int ncycles, const int32_t* cycle_len, const int32_t* cycle_verts, double* out_re_im);
/* The same quantity for connected leafless configurations given as EDGE lists, with at most two independent loops (|E| - |V| <= 1): simple cycles, thetas (two
 * vertices of internal degree 3 joined by three chains), dumbbells (two such vertices, each carrying a closed chain, joined by a bridge) and figure-eights (one vertex
 * of internal degree 4 carrying two closed chains).  Configuration c has config_nedges[c] edges (edge_u[i], edge_v[i]), the lists one after the other;
 * out_re_im[2c, 2c+1] = W(c): the double-layer tensors of its vertices, the cache's messages on every leg that leaves it, the antiprojector on every edge of it.
 * Order and orientation of the edges do not matter: the list is put into a canonical form first.  A simple cycle is handed to the code of tnqs_loop_weights as the
 * ring that starts at its lowest vertex and goes on to the lower of that vertex's two ring neighbours (bit-identical to that call).
 * Precondition, pending gates and scales, unset messages and batching as for tnqs_loop_weights; the workspace of every configuration is computed before anything is
 * allocated.  nconfigs = 0 is allowed.
 * TNQS_ERR_INVALID: an edge that is not in the graph, a repeated edge, a disconnected set, a vertex of internal degree 1, null pointers with nconfigs > 0;
 * TNQS_ERR_UNSUPPORTED: more than two independent loops, sharded handles, vertex degree > 7, a configuration whose workspace exceeds the free device memory, the bytes the
 * handle's own pool holds from earlier calls counted as free (the message names the bytes). */
int tnqs_config_weights(tnqs_handle h, int nconfigs, const int32_t* config_nedges, const int32_t* edge_u, const int32_t* edge_v, double* out_re_im);

/* ---- overlap of two states ---------------------------------------------------------------------------------------
 * inner(psi, phi; alg = "bp") (src/inner.jl:65-69): BP on BilinearForm(ket, bra).  out_log_re_im = the reference's freenergy
 * (complex log of the overlap, imaginary part in (-pi, pi]); the overlap is its exp.  Neither handle's messages are read or written.
 * The conjugate is on the SECOND argument: the value is sum psi conj(phi), what the reference's code computes (bra = dag(prime(phi))) whatever its docstring says.
 * The two handles share graph (vertex and edge lists as given to tnqs_create), CURRENT site dimensions, element type and device; bond dimensions are free per handle
 * and edge, up to 64.  The form's messages are chi_ket(e) x chi_bra(e) matrices m[a + chi_ket b] that live in buffers of the call, the rectangular delta to begin with;
 * sweeps are Gauss-Seidel over the sequence of bp_opts, exactly as tnqs_bp_update runs them (same default sequence, same level schedule), every message absorbed on the
 * ket's side; message_diff is averaged over the sequence.  opts == NULL: the reference's defaults for a bare `update` of the form cache -- maxiter 25 (1 on a tree), NO
 * tolerance, default sequence (a NaN tolerance in opts selects 1e-5 / 1e-8 as in tnqs_bp_update).  Without a tolerance the host is not consulted between sweeps and
 * *final_diff is the last sweep's average; with one there is one read-back per sweep.  Non-convergence is not an error: *niter == maxiter, *final_diff returned.
 * Scalars are f64 whatever the element type: log z = sum_v log(vertex scalar) - sum_e log(edge scalar), complex logs.  A vertex or edge scalar that is exactly zero
 * gives (-inf, 0) (the reference's free energy is -Inf, the overlap 0); a NaN or infinite scalar is TNQS_ERR_NUMERIC.  ket == bra is allowed.  Deferred one-site gates
 * of both handles are applied first (as tnqs_rdm_1site does), pending scale factors are honoured; the work runs on the ket's stream, behind whatever the bra's holds.
 * TNQS_ERR_UNSUPPORTED: a sharded handle, a bond dimension above 64 (the rectangular Gram kernel takes 1..64; there is no scalar form);
 * TNQS_ERR_INVALID: different vertex / edge lists, site dimensions, element types or devices, a null pointer -- all before any device work.
 * niter, final_diff may be NULL. */
int tnqs_inner_bp(tnqs_handle ket, tnqs_handle bra, const tnqs_bp_opts* opts, double* out_log_re_im, int* niter, double* final_diff);

/* ---- amplitudes of bitstrings --------------------------------------------------------------------------------------
 * log <x|psi> of nstrings bitstrings in ONE call, by belief propagation on the single-layer network A_v = T_v[x_v, ...] (the reference's contract(tn; alg = "bp"),
 * src/contract.jl:7-9; what certify_sample contracts per sample, src/sampling.jl:258-285).  configs: nstrings x nv int32, string-major, vertex order of tnqs_create,
 * 0 <= x_v < d_v (the CURRENT site dimension).  The state is taken as it stands on the handle, un-normalised: deferred one-site gates are applied first, pending scale
 * factors are honoured; the handle's own messages are neither read nor written.  Messages are vectors of length chi(e) in the state's type that live in buffers of the
 * call and start as ALL ONES (src/TensorNetworks/tensornetwork.jl:62-64) -- not e_0, which is what tnqs_inner_bp's rectangular delta gives a chi = 1 bra: same fixed
 * points, different numbers after finitely many sweeps on a loopy graph.  Update: m_{u->v}[j] = sum A_u[.., j, ..] prod_{k != v} m_{k->u}[i_k], divided by its element
 * sum when opts->normalize and that sum is not exactly zero; sweeps are Gauss-Seidel over the sequence of bp_opts exactly as tnqs_inner_bp runs them; message_diff is
 * averaged over the sequence.  opts == NULL: maxiter 25 (1 on a tree), NO tolerance, default sequence (a NaN tolerance in opts selects 1e-5 / 1e-8).
 * out_log_re_im[2 n, 2 n + 1] = sum_v log(vertex scalar) - sum_e log(edge scalar) of string n, complex logs in f64 whatever the element type, imaginary part in
 * (-pi, pi]; the amplitude is its exp.  niter[n], final_diff[n], flags[n] (each may be NULL): with a tolerance string n stops at the first sweep whose average diff is
 * <= tolerance and its messages are frozen from then on, so all three and the result are what a call with that string alone gives (one read-back of the done flags per
 * sweep; without a tolerance one read-back per call).  flags bit 0: a vertex or edge scalar of the string is exactly zero, its result is (-inf, 0); bit 1: a scalar is
 * not finite, its result is (NaN, NaN).  Neither fails the call nor touches the other strings.  nstrings == 0: TNQS_OK, nothing done.
 * TNQS_ERR_INVALID, before any device work: a null pointer with work to do, a configuration outside 0 .. d_v - 1, a null explicit sequence, nstrings < 0.
 * TNQS_ERR_UNSUPPORTED: a sharded handle, a vertex of more than 7 neighbours, a bond dimension above 64 (refused up front: the kernels take 1..64 and there is no
 * scalar form), a site tensor of more than 2^30 d_v elements. */
int tnqs_amplitudes_bp(tnqs_handle h, int nstrings, const int32_t* configs, const tnqs_bp_opts* opts, double* out_log_re_im, int32_t* niter, double* final_diff, int32_t* flags);

/* ---- boundary MPS ---------------------------------------------------------------------------------------------------
 * expect(psi, obs; alg = "boundarymps") and norm_sqr(psi; alg = "boundarymps") (src/expect.jl:84-156, src/norm_sqr.jl:86-91, src/MessagePassing/boundarympscache.jl)
 * in ONE call, for a state on an open rectangular grid.  vertex_row / vertex_col: the two coordinates of every vertex, in the vertex order of tnqs_create.
 * partition_by 0 ("row") groups the vertices by vertex_row and orders a group by vertex_col, 1 ("col") the other way round (BoundaryMPSCache, :145-175).  Between
 * neighbouring partitions there is one MPS per direction with one tensor M[l, a, a', r] per cross edge (a / a' = the ket / bra leg of the edge) and link dimensions
 * min(x1^2, x2^2, mps_bond_dimension) (virtual_index_dimension, :119-143); it starts as delta(a, a') times all-ones links and is fitted ONCE (the quotient graph is a
 * line) by the "fitting" update (:330-369): QR gauge walk, one-site sweeps there and back, at most niters sweeps (<= 0: 50), stopping when |cf - previous cf| <
 * tolerance (tolerance < 0: never, NaN: 1e-5 for ComplexF32 / 1e-8 for ComplexF64; one read-back per sweep with a tolerance, none without); normalize != 0 divides
 * every fitted tensor by its norm.  Only the messages the request needs are fitted.  Observable i has obs_nverts[i] support vertices (listed one after the other in
 * obs_verts, all in ONE partition) and one d x d complex128 column-major matrix op[s' + d s] per support vertex in obs_ops, as tnqs_expect_region takes them;
 * out_numer_denom[4 i ..] = {Re, Im numerator, Re, Im denominator} (path_contract, :616-667; the environments of a partition are built once and shared by its
 * observables).  out_log_norm_sqr (may be NULL; with nobs = 0 this is the norm): {Re, Im} of log Z = sum_partitions log(vertex scalar) - sum_quotient edges
 * log(edge scalar) (:504-519), f64 complex logs, imaginary part in (-pi, pi], (-inf, 0) when a scalar is exactly zero.  out_fit_sweeps / out_fit_eps (may be NULL):
 * 2 (P - 1) entries for P partitions, entry p for the message p -> p + 1, entry P - 1 + p for p + 1 -> p: sweeps run and the last |cf - previous cf| (0 sweeps and NaN
 * for a message the request did not need).  The handle's site tensors and BP messages are not changed (deferred one-site gates and pending scale factors are applied
 * first, as tnqs_rdm_1site does); messages and environments live in buffers of the call.
 * LIMITS (TNQS_ERR_UNSUPPORTED before any device work, tnqs_last_error names the limit): bond dimension chi <= 8 with every link <= 64, or chi <= 16 with every link
 * <= 16, a link being min(x1^2, x2^2, mps_bond_dimension) (so chi <= 8 with mps_bond_dimension <= 64 and chi <= 16 with mps_bond_dimension <= 16 are always taken, and a
 * larger mps_bond_dimension is taken where no link of the network reaches it); site dimension <= 16; sharded handles are refused.
 * TNQS_ERR_INVALID (before any device work): a graph that is not an open rectangular grid under the partitioning -- it would need pseudo-edges, its partitions form
 * a ring, a partition is not a path --, fewer than two partitions or two vertices per partition, a support outside one partition, a repeated or bad vertex, null pointers,
 * mps_bond_dimension < 1. */
typedef struct {
    int partition_by;         /* 0: "row", 1: "col" */
    int mps_bond_dimension;   /* R >= 1 */
    int niters;               /* <= 0: 50 */
    double tolerance;         /* < 0: none, NaN: default_tolerance of the element type */
    int normalize;
} tnqs_bmps_opts;
int tnqs_expect_bmps(tnqs_handle h, const tnqs_bmps_opts* opts, const int32_t* vertex_row, const int32_t* vertex_col,
                     int nobs, const int32_t* obs_nverts, const int32_t* obs_verts, const double* obs_ops,
                     double* out_numer_denom, double* out_log_norm_sqr, int32_t* out_fit_sweeps, double* out_fit_eps);

/* ---- multi-GPU sharding (no reference analogue).  A rank owns a vertex subset: it holds only
 *      those site tensors and does all per-vertex work for them; messages are replicated.  The library calls
 *      the host-supplied all-gather at the exchange points (host side: torch.distributed over RCCL). --------- */
/* all-gather over the ranks of `bytes_per_rank` bytes: rank r's block sits at exch_base + r*bytes_per_rank of the
 * exchange buffer handed to tnqs_set_sharding (in place).  Must be complete (device-visible) on return. */
typedef int (*tnqs_allgather_fn)(void* ctx, void* exch_base, int64_t bytes_per_rank, int nranks);
/* vertex_owner[v] in [0, nranks).  exch_dev/exch_bytes: a device buffer owned by the host side (e.g. a torch tensor)
 * that the library packs its exchange payloads into.  Call right after tnqs_create on every rank; site tensors of
 * vertices owned by other ranks are dropped, and tnqs_set_site_tensor on them only records the bond dimensions
 * (host may be NULL).  Exchanges per apply_gates call: one per BP level (raw messages, <= 2|E| chi^2 elements per
 * sweep in total) and two per gate batch (the d*chi x d*chi Gram matrices; chi', truncation error, S and X2). */
int tnqs_set_sharding(tnqs_handle h, int rank, int nranks, const int32_t* vertex_owner, tnqs_allgather_fn fn, void* ctx,
                      void* exch_dev, int64_t exch_bytes);

/* The same sharding with the transport INSIDE the library: RCCL (librccl.so, loaded at run time) over xGMI.  One rank calls
 * tnqs_rccl_unique_id and hands the 128 opaque bytes (an ncclUniqueId) to every rank by whatever means the host has (MPI, a file,
 * torch.distributed's store); every rank then calls tnqs_set_sharding_rccl right after tnqs_create -- it joins the communicator
 * (collective: blocks until all nranks ranks have called) and allocates the exchange buffer (exch_bytes, on the handle's device).
 * From then on every exchange point is ONE in-place ncclAllGather enqueued on the handle's stream: no stream synchronisation, no
 * host callback.  Copies of the handle share the communicator; it is destroyed with the last of them.  nranks == 1 is allowed
 * (nothing is exchanged). */
int tnqs_rccl_unique_id(void* out_128_bytes);
int tnqs_set_sharding_rccl(tnqs_handle h, int rank, int nranks, const int32_t* vertex_owner, const void* unique_id_128_bytes,
                           int64_t exch_bytes);
/* all-gathers issued through RCCL by this handle and its copies, and the bytes they gathered (0 in callback mode) */
int tnqs_sharding_stats(tnqs_handle h, int64_t* n_exchanges, int64_t* bytes_exchanged);
/* one-rank round trip through RCCL on `device` (unique id, communicator, in-place all-gather of `bytes` bytes, teardown): lets a
 * single-GPU box check that the transport loads and runs -- RCCL refuses two ranks on one GPU */
int tnqs_rccl_selftest(int device, int64_t bytes);
/* LOCAL preflight, no collective: librccl.so loads and exports every entry point the transport uses.  A host that is about to call
 * tnqs_set_sharding_rccl on N ranks runs this (or tnqs_rccl_selftest) on every rank first and lets the ranks AGREE on the outcome over
 * a channel it already trusts, so that no rank enters the communicator set-up while another one has already failed. */
int tnqs_rccl_preflight(void);

/* ---- profiling: HIP-event timing of the kernel classes on the handle's stream ---------------------------- */
enum { TNQS_PROF_BP_MODEPROD = 0, TNQS_PROF_BP_GRAM = 1, TNQS_PROF_GATE_MODEPROD = 2, TNQS_PROF_GATE_GRAM = 3,
       TNQS_PROF_GATE_APPLY = 4, TNQS_PROF_JACOBI = 5, TNQS_PROF_SMALL = 6, TNQS_PROF_BP_FUSED = 7, TNQS_PROF_BP_PAIR = 8, TNQS_PROF_BP_PAIRGRAM = 9,
       /* whole phases, first to last kernel on the handle's stream (side streams join it before a phase ends): the CRITICAL-PATH time of the BP updates (launches =
        * sweeps) and of the batches of two-site gates (launches = batches) -- the kernel classes above overlap each other where a phase runs on two streams */
       TNQS_PROF_PHASE_BP_UPDATE = 10, TNQS_PROF_PHASE_GATE_BATCH = 11,
       /* every launch of tnqs_loop_weights and tnqs_config_weights; flops: 8 m n k per complex product of the batched GEMM */
       TNQS_PROF_LOOP = 12,
       /* the bond-contraction kernel of tnqs_rdm_edges (its chains and Grams are booked under TNQS_PROF_SMALL, as the one-site probe's); bytes: Gram partials read + matrices
        * written, flops: 8 chi^2 (d_u d_v)^2 per bond */
       TNQS_PROF_EDGE_RDM = 13,
       /* the apply kernel and the bond contractions of tnqs_rdm_paths (its transfer matrices are booked under TNQS_PROF_LOOP, its chains and Grams under TNQS_PROF_SMALL);
        * bytes: T read + L read + L written / partials read + matrices written, flops: 8 d^2 chi_a^2 chi_b^2 per step, 8 chi^2 (d_u d_w)^2 per pair */
       TNQS_PROF_PATH_RDM = 14, TNQS_PROF_NCLASSES = 15 };
int tnqs_profile_enable(tnqs_handle h, int on);
/* launches, total ms, algorithmic bytes (min traffic: operands read once + result written once) and flops */
int tnqs_profile_get(tnqs_handle h, int cls, int64_t* launches, double* total_ms, double* alg_bytes, double* alg_flops);
int tnqs_profile_reset(tnqs_handle h);

#ifdef __cplusplus
}
#endif
#endif /* TNQS_H */
