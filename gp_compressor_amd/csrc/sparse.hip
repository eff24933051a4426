// sparse.hip -- the ADD path of the batched online sparse GP (Csato-Opper) : sparse_gp<rbf_kernel, gaussian_noise> and
// sparse_gp_field<rbf_kernel, gaussian_noise_3d> of the reference, one patch per workgroup.
//
// Follows /root/reference/src/sparse_gp.hpp:89-249 (add), :252-295 (delete_bv), :299-351 (predict) and the
// field variant /root/reference/src/sparse_gp_field.hpp:59-215, 219-263, 268-320.  The recursion is strictly
// sequential in the points of one patch and data-dependent (sparse vs full update, capacity / geometric
// deletions), so the parallelism is: patches across workgroups, and inside a patch the O(b) kernel vector, the
// two O(b^2) mat-vecs (C k, Q k) and the O(b^2) rank-1 updates across the 256 threads of the workgroup.  All
// branch decisions are taken from values every thread computes identically (LDS-reduced), so control flow is
// workgroup-uniform.
//
// State layout in HBM (persistent across calls, /root/reference/src/gp_mapping.cpp:338-339 keeps adding to
// trained GPs):  alpha [P][ny][ld], C [P][ld][ld], Q [P][ld][ld] column-major like Eigen, BV [P][ld][2] (AoS,
// = Eigen 2 x b column-major), b [P], total_count [P];  ld = capacity + 1 rounded up to 16 (a full update may hold capacity+1
// basis vectors until the deletion that follows it), or GPC_MAX_BV when capacity == -1.
//
// The helpers it shares with rate control (the block-wide sums and arg-min, the passes over C and Q, delete_bv) are in sparse_device.h,
// the prune / quantise kernels in sparse_rate.hip, the predict / likelihood / train kernels in sparse_predict.hip, the gpc_sparse_* entry
// points in sparse_api.hip.
#include <algorithm>
#include <cstdlib>

#include "sparse_device.h"

// Full update (sparse_gp.hpp:164-203) FUSED with the capacity deletion that must follow it when the basis is full
// (:206-223 -> delete_bv :252-295): the rank-1 growth C' = [C 0; 0 0] + r s s^T, Q' = [Q 0; 0 0] + e e^T / gamma and the
// rank-2 downdate of delete_bv touch every element of C and Q; run back to back they read and write both matrices twice
// (3.2 MB per point at b = 200, and the add path is HBM-bound).  Here the deletion candidate is scored on the updated
// diagonals, the two columns delete_bv needs (loc and the new last one) are formed from the OLD matrices plus the
// rank-1 terms, and one pass writes the final C and Q.  Every element goes through the same floating-point operations
// in the same order as the two-pass form, so the result is the same to the last bit; only the intermediate (b+1) x (b+1)
// matrices never reach memory.  b == capacity on entry and on return.
// When the coordinates of the NEXT point are known (nxt != nullptr) the pass also forms that point's mat-vecs (sp_rmw_cq_next).
template <int RB, bool TRI = false, bool PK = false>
__device__ static int sp_full_update_delete(const SpState& S, int b, double rr, double gamma, const double* qv, double px0, double px1,
                                            int field_bug, const double* ck, double* eh, double* sv, double* Cstar, double* Qstar,
                                            double* Crep, double* Qrep, double* anew, double* sval, int* sidx,
                                            const double* nxt, double* kvn, double* pnext, double sf, double c_exp, const double* T,
                                            double* pnext_col = nullptr, bool tri_p = false)
{
    const bool tri = TRI && tri_p;
    const int tid = threadIdx.x, ld = S.ld, ldm = S.ldm, ny = S.ny, last = b;
    const double ig = (double)1.0f / gamma;
    for (int i = tid; i <= b; i += SP_NTH) {
        const double si = (i < b) ? ck[i] : (double)1.0f;
        sv[i] = si;
        if (i == b) eh[b] = (double)(-1.0f);
        for (int c = 0; c < ny; ++c) {
            const double a0 = (i < b) ? S.alpha[c * ld + i] : 0.0;
            anew[c * ld + i] = a0 + qv[c] * si;
        }
    }
    __syncthreads();
    // capacity deletion candidate on the updated state (:206-223): argmin |alpha_i|^2 / (Q_ii + C_ii), first index wins ties
    double best = 0.0;
    int loc = 0x7fffffff;
    bool have = false;
    for (int i = tid; i <= b; i += SP_NTH) {
        double a2 = 0.0;
        for (int c = 0; c < ny; ++c) { const double a = anew[c * ld + i]; a2 += a * a; }
        const double c0 = (i < b) ? S.C[sp_at<PK>(i, i, ldm)] : 0.0, q0 = (i < b) ? S.Q[sp_at<PK>(i, i, ldm)] : 0.0;
        const double cd = c0 + (rr * sv[i]) * sv[i], qd = q0 + (ig * eh[i]) * eh[i];
        const double score = a2 / (qd + cd);
        if (!have || SP_TAKE(score, i, best, loc)) { best = score; loc = i; have = true; }
    }
    if (!have) best = __builtin_inf();
    sp_block_argmin(best, loc, sval, sidx);
    if (loc < 0 || loc > b) loc = 0;
    // columns loc and last of the updated matrices (delete_bv :259-278)
    for (int i = tid; i <= b; i += SP_NTH) {
        const bool old = (i < b) && (loc < b);
        const size_t al = tri ? sp_sym_at<PK>(old ? i : 0, old ? loc : 0, ldm) : (size_t)i + (size_t)loc * ldm;
        const double c0 = old ? S.C[al] : 0.0, q0 = old ? S.Q[al] : 0.0;
        Cstar[i] = c0 + (rr * sv[i]) * sv[loc];
        Qstar[i] = q0 + (ig * eh[i]) * eh[loc];
        Crep[i] = 0.0 + (rr * sv[i]) * sv[b];
        Qrep[i] = 0.0 + (ig * eh[i]) * eh[b];
    }
    __syncthreads();
    const double cstar = Cstar[loc], qstar = Qstar[loc];
    double alphastar[3];
    for (int c = 0; c < ny; ++c) alphastar[c] = anew[c * ld + loc];
    __syncthreads();
    if (tid == 0) {
        Cstar[loc] = Cstar[last];   // (:263)
        Qstar[loc] = Qstar[last];   // (:275)
        Crep[loc] = Crep[last];     // (:267)
        Qrep[loc] = Qrep[last];     // (:278)
    }
    if (tid == 32 && loc != last) {
        S.BV[2 * loc] = px0;        // BV.col(loc) = BV.col(last) = the new point (:291)
        S.BV[2 * loc + 1] = px1;
    }
    __syncthreads();
    const int nb = b;
    const double qc_den = qstar + cstar;
    // alpha (:257, :285; field variant :250-253 multiplies when bug-compatible)
    for (int i = tid; i < nb; i += SP_NTH) {
        const double qc = Qstar[i] + Cstar[i];
        for (int c = 0; c < ny; ++c) {
            const double asw = (i == loc) ? anew[c * ld + last] : anew[c * ld + i];
            if (ny == 1) S.alpha[i] = asw - alphastar[0] / qc_den * qc;
            else S.alpha[c * ld + i] = asw - alphastar[c] * (field_bug ? qc_den * qc : qc / qc_den);
        }
    }
    // the one pass over C and Q
    auto element = [&](int i, int j, double& c, double& q) {
        double bc, bq;
        if (i == loc) { bc = Crep[j]; bq = Qrep[j]; }
        else if (j == loc) { bc = Crep[i]; bq = Qrep[i]; }
        else {
            bc = c + (rr * sv[i]) * sv[j];
            bq = q + (ig * eh[i]) * eh[j];
        }
        const double qq = (Qstar[i] * Qstar[j]) / qstar;
        const double cc = ((Qstar[i] + Cstar[i]) * (Qstar[j] + Cstar[j])) / qc_den;
        c = bc + (qq - cc);
        q = bq - qq;
    };
    if (nxt) {
        // k' against the updated basis (BV[loc] was replaced above, behind a barrier)
        const double n0 = nxt[0], n1 = nxt[1];
        for (int i = tid; i < nb; i += SP_NTH) kvn[i] = gpc_rbf_neg(sf, c_exp, n0, n1, S.BV[2 * i], S.BV[2 * i + 1], T);
        __syncthreads();
        if (tri) sp_tri_pass<1 | 2 | 4, PK>(S.C, S.Q, ldm, ld, nb, kvn, pnext, pnext_col, element);
        else sp_rmw_cq_next<true, RB>(S.C, S.Q, ldm, ld, nb, kvn, pnext, element);
    } else {
        if (tri) sp_tri_pass<1 | 2, PK>(S.C, S.Q, ldm, ld, nb, nullptr, nullptr, nullptr, element);
        else sp_rmw_cq<RB>(S.C, S.Q, ldm, nb, element);
    }
    __syncthreads();
    return nb;
}

struct SpAddParams {
    gpc_params prm;
    double c_exp;
    int P, ny, ld, n_total;
    const int32_t* off;
    const double *x0, *x1, *y;
    const int32_t* perm;
    double *alpha, *C, *Q, *BV;
    int32_t *b, *count, *stat, *status_out;
    int fuse_next;   // 1: full-update passes also form the next point's mat-vecs (0 only through GPC_SPARSE_NO_FUSE, for the tests)
    const int32_t* start_it;   // per patch: points of this call already consumed by the small-basis kernel (nullptr: 0)
    int32_t* done_it;          // small-basis kernel only: how many points of this call it consumed
    uint8_t* trace;            // diagnostic: one decision byte per point of the call, in insertion order (or nullptr)
    // work list of the phases after the rows phase: the patches it did not finish, in the order they were handed over.  The kernels
    // that follow take list entries by ticket (one atomic per patch) instead of a static share of all P patches: only a fifth of the
    // patches reach them, and with static shares the wave that happens to own eight of those decides the launch time.
    int32_t* list;             // [P] patch ids (nullptr: static shares)
    int32_t* list_n;           // [0] entries in `list`, [1] .. [3] ticket counters of the launches that draw from it
    int32_t* out_list;         // where a phase that draws from `list` puts what it hands on (round 4: every later phase walks only the
    int32_t* out_list_n;       // entries it has work in, not the first phase's whole list: a ticket costs ~23 ns device-wide), or nullptr
    int ticket_slot;           // which counter this launch draws from
    int tri_min;               // triangular mode (sparse_add_kernel<false, ., true>): for patches that arrive with at least this many basis vectors
};

// Small-basis phase.  With the reference's default hyper-parameters the basis stays at a dozen vectors whatever the capacity,
// and a point is a handful of short loops whose cost is the latency of C and Q in L2 / HBM.  sparse_add_kernel<true> runs one
// wave per patch with C and Q (up to SP_BMAX x SP_BMAX) resident in LDS, ten patches per CU, and hands a patch over -- state written back, the
// number of points consumed recorded in done_it -- at the first point that would grow its basis beyond SP_BMAX; the regular
// kernel then continues from there (start_it).  Same operations in the same order: the two-phase run leaves the states of
// a one-phase run, bit for bit.

// PROBIT: the probit functor (sqrt, erf, exp: ~450 instructions and their constants) is compiled in only where it is used -- in the
// Gaussian instantiation, the reference's production path, its registers go to the point loop
// TRI: the triangular mode of the four-wave shape (see sp_tri_pass)
// RES (round 4; implies TRI): the lower triangles of C and Q of the patch in flight are RESIDENT IN LDS, packed (sp_at<true>), loaded once
// when the patch enters the kernel and written back (both triangles) once when it leaves -- the add call moves 16 b^2 bytes per patch instead
// of 16 b^2 per POINT.  Fits while 2 x (capacity + 1)(capacity + 2) / 2 doubles + the vectors stay within the CU's 160 KB: capacity <= 120,
// which covers the reference's default of 100 (/root/reference/src/sparse_gp.h:48).  One workgroup of four waves per CU.  Every patch runs
// the triangular passes (whatever basis it arrives with); same element updates, same summation order as the HBM-resident triangular mode.
template <bool SMALL, bool PROBIT = false, bool TRI = false, bool RES = false, int BM = SP_BMAX>
__global__ __launch_bounds__(SMALL ? 64 : SP_THREADS, SMALL ? 4 : 2) void sparse_add_kernel(SpAddParams A)   // <= 256 VGPRs (128 for the small-basis phase)
{
    static_assert(!RES || (TRI && !SMALL && !PROBIT), "the LDS-resident mode is a form of the triangular mode");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ldg = A.ld, ny = A.ny;               // ldg: strides of the state in global memory
    const int ld = SMALL ? BM + 1 : ldg;      // stride of the LDS vectors (and of alpha / BV while they live in LDS)
    const int ldm = SMALL ? BM : ldg;         // stride of C and Q where the update loops see them
    constexpr int RB = SMALL ? 2 : SP_RMW;         // elements per thread and trip of the update passes (LDS needs no deep batches)
    double* T = reinterpret_cast<double*>(smem);   // 64
    double* red = T + 64;                          // 16
    double* sval = red + 16;                       // 4
    int* sidx = reinterpret_cast<int*>(sval + 4);  // 4 ints (2 doubles)
    double* kv = sval + 6;                         // k        [ld]
    double* ck = kv + ld;                          // C k      [ld]
    double* eh = ck + ld;                          // e_hat    [ld+1]
    double* sv = eh + ld + 1;                      // s / s_hat[ld+1]
    double* part = sv + ld + 1;                    // partial mat-vec sums [4][2][ld]
    double* Cstar = part;                          // delete_bv scratch aliases the mat-vec partials
    double* Qstar = part + ld;
    double* Crep = part + 2 * ld;
    double* Qrep = part + 3 * ld;
    double* pnext = part + 8 * ld;                 // the NEXT point's mat-vec partials, formed inside the fused update pass
    double* kvn = pnext + 8 * ld;                  // ... and its k  [ld]
    double* alphaL = kvn + ld;                     // alpha [ny][ld] and BV [ld][2] of the patch in flight: read and updated at every
    double* BVL = alphaL + 3 * ld;                 // point, so they live here between the first and the last point of the call
    double* Cl = BVL + 2 * ld;                     // SMALL: C, Q [BM][BM]
    double* Ql = Cl + BM * BM;
    double* part_col = BVL + 2 * ld;               // TRI: column parts of the mat-vecs [2][ld], this point's and the next one's
    double* pnext_col = part_col + 2 * ld;
    const int ldp = A.prm.capacity + 1;            // RES: leading dimension of the packed triangles
    double* Cp = pnext_col + 2 * ld;               // RES: C, Q lower triangles, packed [ldp (ldp + 1) / 2]
    double* Qp = Cp + (ldp * (ldp + 1)) / 2;
    gpc_exp_table_init(T);

    const double sf = A.prm.sigmaf_sq, s20 = A.prm.noise, eps_tol = A.prm.eps_tol;
    const int capacity = A.prm.capacity;

    int* s_ticket = reinterpret_cast<int*>(red + 15);             // (the last slot of the reduction scratch is never used: <= 3 sums x 4 waves)
    for (int slot = blockIdx.x;; slot += gridDim.x) {
        int patch = slot;
        if (A.list) {                                                // work list: the next entry nobody has taken yet
            // (the first entry of a workgroup is its own index: tickets to ONE counter are served at ~23 ns each device-wide -- the
            // 32768 skipped entries of a C4-fill call take 0.76 ms that way -- and at launch every workgroup asks at once)
            int idx = slot;
            if (slot != (int)blockIdx.x) {
                __syncthreads();
                if (tid == 0) *s_ticket = (int)gridDim.x + atomicAdd(A.list_n + A.ticket_slot, 1);
                __syncthreads();
                idx = *s_ticket;
            }
            if (idx >= A.list_n[0]) break;
            patch = A.list[idx];
        } else if (patch >= A.P) {
            break;
        }
        const int o = A.off[patch], n = A.off[patch + 1] - o;
        SpState S;
        S.ld = ld; S.ny = ny; S.ldm = RES ? ldp : ldm;
        double* const alphag = A.alpha + (size_t)patch * ny * ldg;
        double* const BVg = A.BV + (size_t)patch * ldg * 2;
        double* const Cg = A.C + (size_t)patch * ldg * ldg;
        double* const Qg = A.Q + (size_t)patch * ldg * ldg;
        S.alpha = alphaL;
        S.C = RES ? Cp : SMALL ? Cl : Cg;
        S.Q = RES ? Qp : SMALL ? Ql : Qg;
        S.BV = BVL;
        int b = A.b[patch];
        int st = A.stat[patch];
        // the triangular passes pay from a mid-sized basis on (their per-block reductions and the uneven shares of the four waves cost
        // more than half a stream of a small matrix saves): decided per patch and call from the basis it arrives with
        [[maybe_unused]] const bool tri = RES || (TRI && b >= A.tri_min);
        const int it0 = A.start_it ? A.start_it[patch] : 0;     // an earlier phase (rows / small-basis) already took these
        __syncthreads();
        if (SMALL && (b > BM || n == 0)) {          // too large from the start (or nothing to do): all of it is the regular kernel's
            if (tid == 0) {
                A.done_it[patch] = it0;
                if (A.out_list && n > 0 && it0 < n) A.out_list[atomicAdd(A.out_list_n, 1)] = patch;
            }
            continue;
        }
        if (A.start_it && n > 0 && it0 >= n) continue;   // an earlier phase finished this patch (and wrote its state, status and done_it)
        for (int i = tid; i < b; i += SP_NTH) {
            BVL[2 * i] = BVg[2 * i];
            BVL[2 * i + 1] = BVg[2 * i + 1];
            for (int c = 0; c < ny; ++c) alphaL[c * ld + i] = alphag[c * ldg + i];
        }
        if (SMALL) {
            for (int e = tid; e < b * b; e += SP_NTH) {
                const int i = e % b, j = e / b;
                Cl[i + j * BM] = Cg[i + (size_t)j * ldg];
                Ql[i + j * BM] = Qg[i + (size_t)j * ldg];
            }
        }
        if (RES) {                                       // the lower triangles come on chip (the upper ones are redundant: every producer mirrors)
            for (int e = tid; e < b * b; e += SP_NTH) {
                const int i = e % b, j = e / b;
                if (i >= j) {
                    Cp[sp_at<true>(i, j, ldp)] = Cg[i + (size_t)j * ldg];
                    Qp[sp_at<true>(i, j, ldp)] = Qg[i + (size_t)j * ldg];
                }
            }
        }
        int it_end = n;                                  // SMALL: where this phase stopped
        __syncthreads();

        bool have_next = false;                      // k and the mat-vec partials of this iteration's point were formed by the previous one
        // The coordinates and targets of a point sit behind two dependent global loads (insertion order, then the point): they
        // are fetched one point ahead, and the index two ahead, so that nothing of a point waits on them (in the small-basis
        // regime those round trips were a quarter of a point).
        double cx0 = 0.0, cx1 = 0.0, cy[3] = {0.0, 0.0, 0.0};       // the current point
        int r_nxt = 0;                                                // row of point it + 1
        if (it0 < n) {
            const int r0 = A.perm ? A.perm[o + it0] : it0;
            cx0 = A.x0[o + r0];
            cx1 = A.x1[o + r0];
            for (int c = 0; c < ny; ++c) cy[c] = A.y[(size_t)c * A.n_total + o + r0];
            if (it0 + 1 < n) r_nxt = A.perm ? A.perm[o + it0 + 1] : it0 + 1;
        }
        double nx0 = 0.0, nx1 = 0.0, nyv[3] = {0.0, 0.0, 0.0};      // point it + 1, in flight
        int r_nxt2 = 0;
        for (int it = it0; it < n; ++it, cx0 = nx0, cx1 = nx1, cy[0] = nyv[0], cy[1] = nyv[1], cy[2] = nyv[2], r_nxt = r_nxt2) {
            const double px0 = cx0, px1 = cx1;
            double yv[3] = {cy[0], cy[1], cy[2]};
            const bool more_pts = it + 1 < n;
            if (more_pts) {
                nx0 = A.x0[o + r_nxt];
                nx1 = A.x1[o + r_nxt];
                for (int c = 0; c < ny; ++c) nyv[c] = A.y[(size_t)c * A.n_total + o + r_nxt];
                if (it + 2 < n) r_nxt2 = A.perm ? A.perm[o + it + 2] : it + 2;
            }
            const double kstar = sp_kstar(sf, px0, px1);   // kernel_function(X, X)  (:98)

            const bool from_prev = have_next;
            have_next = false;
            if (b == 0) {
                // First point (:100-114)
                if (tid == 0) {
                    for (int c = 0; c < ny; ++c) S.alpha[c * ld] = yv[c] / (kstar + s20);
                    S.C[0] = (double)(-1.0f) / (kstar + s20);
                    S.Q[0] = (double)(1.0f) / kstar;
                    S.BV[0] = px0;
                    S.BV[1] = px1;
                }
                b = 1;
                {   // isnan(C(0,0)) (:245) runs after the first point too: NaN when k* is (a coordinate NaN or +-inf)
                    const double c00 = (double)(-1.0f) / (kstar + s20);
                    if (c00 != c00 && st == GPC_STATUS_OK) st = GPC_STATUS_NAN;
                }
                if (A.trace && tid == 0) A.trace[o + it] = 0x81;
                __syncthreads();
                continue;
            }
            int dec = 0;     // decision byte (include/gpc.h, gpc_sparse_set_trace): bit 0 full update, bits 1-3 / 4-6 deletions

            // k = construct_covariance(X, BV)  (:119, :523-530)
            if (from_prev) {
                double* t_ = kv; kv = kvn; kvn = t_;       // formed with the update pass of the previous point
            } else {
                for (int i = tid; i < b; i += SP_NTH) kv[i] = gpc_rbf_neg(sf, A.c_exp, px0, px1, S.BV[2 * i], S.BV[2 * i + 1], T);
            }
            __syncthreads();

            // C k and e_hat = Q k (:140,:160,:171): wave w covers columns j in its quarter, lanes cover rows
            const double* pp = from_prev ? pnext : part;
            [[maybe_unused]] const double* pc = from_prev ? pnext_col : part_col;
            if (TRI && tri && !from_prev) {
                sp_tri_pass<4, RES>(S.C, S.Q, S.ldm, ld, b, kv, part, part_col, [](int, int, double&, double&) {});
            } else if (!from_prev && SMALL && b <= 32) {
                // one wave, small basis: the four quarters side by side (see sp_rmw_cq_next)
                const int shift = b <= 16 ? 4 : 5;
                const int i = lane & ((1 << shift) - 1), G = 64 >> shift;
                for (int quarter = lane >> shift; quarter < 4; quarter += G) {
                    const int jlo = (b * quarter) >> 2, jhi = (b * (quarter + 1)) >> 2;
                    double ac = 0.0, aq = 0.0;
                    if (i < b) {
                        for (int j = jlo; j < jhi; ++j) {
                            const double kj = kv[j];
                            ac += S.C[i + (size_t)j * ldm] * kj;
                            aq += S.Q[i + (size_t)j * ldm] * kj;
                        }
                        part[(quarter * 2 + 0) * ld + i] = ac;
                        part[(quarter * 2 + 1) * ld + i] = aq;
                    }
                }
            } else if (!from_prev) {
                for (int quarter = wave; quarter < 4; quarter += SP_NTH >> 6) {     // one quarter per wave, or all four in turn
                    const int jlo = (b * quarter) >> 2, jhi = (b * (quarter + 1)) >> 2;
                    for (int i = lane; i < b; i += 64) {
                        double ac = 0.0, aq = 0.0;
                        for (int j = jlo; j < jhi; ++j) {
                            const double kj = kv[j];
                            ac += S.C[i + (size_t)j * ldm] * kj;
                            aq += S.Q[i + (size_t)j * ldm] * kj;
                        }
                        part[(quarter * 2 + 0) * ld + i] = ac;
                        part[(quarter * 2 + 1) * ld + i] = aq;
                    }
                }
            }
            __syncthreads();
            double sums[4] = {0.0, 0.0, 0.0, 0.0};   // m[0..2] partial, (kCk, ke) handled in a second pass
            double dots[4] = {0.0, 0.0, 0.0, 0.0};
            for (int i = tid; i < b; i += SP_NTH) {
                double c_ = pp[0 * ld + i] + pp[2 * ld + i] + pp[4 * ld + i] + pp[6 * ld + i];
                double q_ = pp[1 * ld + i] + pp[3 * ld + i] + pp[5 * ld + i] + pp[7 * ld + i];
                if (TRI && tri) {                            // + the column part: rows below the diagonal
                    c_ += pc[i];
                    q_ += pc[ld + i];
                }
                ck[i] = c_;
                eh[i] = q_;
                const double ki = kv[i];
                dots[0] += ki * c_;                        // k^T C k   (:122)
                dots[1] += ki * q_;                        // k^T e_hat (:144)
                for (int c = 0; c < ny; ++c) sums[c] += S.alpha[c * ld + i] * ki;   // m = alpha^T k (:121)
            }
            sp_block_sum4<2>(dots, red);
            if (ny == 1) sp_block_sum4<1>(sums, red);
            else sp_block_sum4<3>(sums, red);
            const double s2 = kstar + dots[0];
            double gamma = kstar - dots[1];
            if (gamma < (double)1e-12f) gamma = 0;          // :146-151

            // r = noise.dx2_ln, q = noise.dx_ln  (/root/reference/src/gaussian_noise.cpp:9-18, gaussian_noise_3d.cpp:11-20,
            // probit_noise.cpp:11-31)
            double rr, qv[3];
            if (PROBIT && A.prm.noise_model != GPC_NOISE_GAUSSIAN && ny == 1) {
                if constexpr (PROBIT) gpc_probit_q_r(A.prm.noise_model, s20, yv[0], sums[0], s2, &qv[0], &rr);
            } else {
                rr = (double)(-1.0f) / (s20 + s2);
                for (int c = 0; c < ny; ++c) qv[c] = (yv[c] - sums[c]) / (s20 + s2);
            }

            if (gamma < eps_tol && capacity != -1) {
                // sparse update (:155-163)
                const double eta = 1 / (1 + gamma * rr);
                for (int i = tid; i < b; i += SP_NTH) {
                    const double sh = ck[i] + eh[i];        // s_hat = C*k + e_hat
                    sv[i] = sh;
                    for (int c = 0; c < ny; ++c) S.alpha[c * ld + i] += sh * (qv[c] * eta);
                }
                __syncthreads();
                const double re = rr * eta;
                if (A.fuse_next && it + 1 < n) {
                    // the basis does not change: the next point's k against it, and its mat-vecs out of this pass (Q is only read)
                    const double n0 = nx0, n1 = nx1;
                    for (int i = tid; i < b; i += SP_NTH) kvn[i] = gpc_rbf_neg(sf, A.c_exp, n0, n1, S.BV[2 * i], S.BV[2 * i + 1], T);
                    __syncthreads();
                    auto proj = [&](int i, int j, double& c, double&) { c = c + (re * sv[i]) * sv[j]; };
                    if (TRI && tri) sp_tri_pass<1 | 4, RES>(S.C, S.Q, S.ldm, ld, b, kvn, pnext, pnext_col, proj);
                    else sp_rmw_cq_next<false, RB>(S.C, S.Q, ldm, ld, b, kvn, pnext, proj);
                    have_next = true;
                } else if (TRI && tri) {
                    sp_tri_pass<1 | 8, RES>(S.C, S.Q, S.ldm, ld, b, nullptr, nullptr, nullptr, [&](int i, int j, double& c, double&) { c = c + (re * sv[i]) * sv[j]; });
                } else {
                    const int nn = b * b;
                    for (int e0 = tid; e0 < nn; e0 += SP_NTH * RB) {     // loads first, see sp_rmw_cq
                        double cv[RB];
                        int ii[RB], jj[RB];
#pragma unroll
                        for (int u = 0; u < RB; ++u) {
                            const int e = e0 + u * SP_NTH, ec = e < nn ? e : e0;
                            ii[u] = ec % b;
                            jj[u] = ec / b;
                            cv[u] = S.C[ii[u] + (size_t)jj[u] * ldm];
                        }
#pragma unroll
                        for (int u = 0; u < RB; ++u)
                            if (e0 + u * SP_NTH < nn) S.C[ii[u] + (size_t)jj[u] * ldm] = cv[u] + (re * sv[ii[u]]) * sv[jj[u]];
                    }
                }
                __syncthreads();
            } else if (SMALL && b + 1 > BM && !(capacity > 0 && capacity <= BM)) {
                it_end = it;                                // this point would grow the basis beyond the resident block: nothing of it
                break;                                      // has been applied yet -- the regular kernel redoes it from the state as it is
            } else if (b >= ldg) {
                st = GPC_STATUS_OVERFLOW;                   // capacity == -1 and GPC_MAX_BV reached: skip the point
            } else if (capacity > 0 && b + 1 > capacity) {
                // full update + the capacity deletion it forces, in one pass over C and Q
                double nx[2] = {0.0, 0.0};
                const bool more = A.fuse_next && it + 1 < n;
                if (more) {
                    nx[0] = nx0;
                    nx[1] = nx1;
                }
                b = sp_full_update_delete<RB, TRI, RES>(S, b, rr, gamma, qv, px0, px1, A.prm.ref_field_delete_bug, ck, eh, sv, Cstar, Qstar, Crep,
                                               Qrep, part + 4 * ld, sval, sidx, more ? nx : nullptr, kvn, pnext, sf, A.c_exp, T, pnext_col, tri);
                have_next = more;
                dec = 1 | 2;
            } else {
                // full update (:164-203)
                dec = 1;
                for (int i = tid; i <= b; i += SP_NTH) {
                    const double si = (i < b) ? ck[i] : (double)1.0f;
                    sv[i] = si;
                    if (i == b) eh[b] = (double)(-1.0f);
                    for (int c = 0; c < ny; ++c) {
                        const double a0 = (i < b) ? S.alpha[c * ld + i] : 0.0;
                        S.alpha[c * ld + i] = a0 + qv[c] * si;
                    }
                }
                if (tid == 64 % SP_NTH) {
                    S.BV[2 * b] = px0;
                    S.BV[2 * b + 1] = px1;
                }
                __syncthreads();
                const double ig = (double)1.0f / gamma;
                const int nb = b + 1;
                auto grow = [&](int i, int j, double& c, double& q) {
                    const bool old = (i < b) && (j < b);          // the new row / column starts from zero, whatever memory held
                    c = (old ? c : 0.0) + (rr * sv[i]) * sv[j];
                    q = (old ? q : 0.0) + (ig * eh[i]) * eh[j];
                };
                if (A.fuse_next && it + 1 < n) {
                    // the next point's k against the grown basis, and its mat-vecs out of this pass
                    const double n0 = nx0, n1 = nx1;
                    for (int i = tid; i < nb; i += SP_NTH) kvn[i] = gpc_rbf_neg(sf, A.c_exp, n0, n1, S.BV[2 * i], S.BV[2 * i + 1], T);
                    __syncthreads();
                    if (TRI && tri) sp_tri_pass<1 | 2 | 4, RES>(S.C, S.Q, S.ldm, ld, nb, kvn, pnext, pnext_col, grow);
                    else sp_rmw_cq_next<true, RB>(S.C, S.Q, ldm, ld, nb, kvn, pnext, grow);
                    have_next = true;
                } else {
                    if (TRI && tri) sp_tri_pass<1 | 2, RES>(S.C, S.Q, S.ldm, ld, nb, nullptr, nullptr, nullptr, grow);
                    else sp_rmw_cq<RB>(S.C, S.Q, ldm, nb, grow);
                }
                b = nb;
                __syncthreads();
            }

            // Delete BVs if necessary (:206-223)
            while (b > capacity && capacity > 0) {
                double best = 0.0;
                int loc = 0x7fffffff;
                bool have = false;
                for (int i = tid; i < b; i += SP_NTH) {
                    double a2 = 0.0;
                    for (int c = 0; c < ny; ++c) { const double a = S.alpha[c * ld + i]; a2 += a * a; }
                    const double score = a2 / (S.Q[sp_at<RES>(i, i, S.ldm)] + S.C[sp_at<RES>(i, i, S.ldm)]);
                    if (!have || SP_TAKE(score, i, best, loc)) { best = score; loc = i; have = true; }
                }
                if (!have) best = __builtin_inf();
                sp_block_argmin(best, loc, sval, sidx);
                if (loc < 0 || loc >= b) loc = 0;
                b = sp_delete_bv<RB, TRI, RES>(S, b, loc, A.prm.ref_field_delete_bug, Cstar, Qstar, Crep, Qrep, tri);
                have_next = false;
                if (((dec >> 1) & 7) < 7) dec += 2;
            }
            // Delete for geometric reasons (:226-242)
            {
                double minscore = 0.0;
                while (minscore < (double)1e-9f && b > 1) {
                    double best = 0.0;
                    int loc = 0x7fffffff;
                    bool have = false;
                    for (int i = tid; i < b; i += SP_NTH) {
                        const double score = (double)1.0f / S.Q[sp_at<RES>(i, i, S.ldm)];
                        if (!have || SP_TAKE(score, i, best, loc)) { best = score; loc = i; have = true; }
                    }
                    if (!have) best = __builtin_inf();
                    // one wave: if no lane holds a score below the threshold the loop ends whatever the minimum is (>= 1e-9f, or NaN:
                    // both leave it, nothing else reads minscore) -- the arg-min is only needed to find WHICH vector goes
                    if (SP_NTH == 64 && __builtin_amdgcn_ballot_w64(have && best < (double)1e-9f) == 0) break;
                    sp_block_argmin(best, loc, sval, sidx);
                    if (loc < 0 || loc >= b) loc = 0;
                    minscore = best;
                    if (minscore < (double)1e-9f) {
                        b = sp_delete_bv<RB, TRI, RES>(S, b, loc, A.prm.ref_field_delete_bug, Cstar, Qstar, Crep, Qrep, tri);
                        have_next = false;              // the matrices and the basis changed after the pass
                        if (((dec >> 4) & 7) < 7) dec += 16;
                    }
                    else if (!(minscore >= (double)1e-9f)) break;   // NaN: `minscore < 1e-9f` is false in the reference too
                }
            }
            // isnan(C(0,0)) -> "sparse_gp::C has become Nan" (:245)
            {
                const double c00 = S.C[0];
                if (c00 != c00 && st == GPC_STATUS_OK) st = GPC_STATUS_NAN;
            }
            if (A.trace && tid == 0) A.trace[o + it] = (uint8_t)dec;
        }
        __syncthreads();
        for (int i = tid; i < b; i += SP_NTH) {
            BVg[2 * i] = BVL[2 * i];
            BVg[2 * i + 1] = BVL[2 * i + 1];
            for (int c = 0; c < ny; ++c) alphag[c * ldg + i] = alphaL[c * ld + i];
        }
        if (SMALL) {
            for (int e = tid; e < b * b; e += SP_NTH) {
                const int i = e % b, j = e / b;
                Cg[i + (size_t)j * ldg] = Cl[i + j * BM];
                Qg[i + (size_t)j * ldg] = Ql[i + j * BM];
            }
            if (tid == 0) {
                A.done_it[patch] = it_end;
                if (A.out_list && it_end < n) A.out_list[atomicAdd(A.out_list_n, 1)] = patch;      // handed on: the next phase continues it
            }
        }
        if (RES) {
            // the state goes back to HBM, both triangles (every other kernel reads full matrices): 16 b^2 bytes once per call
            for (int e = tid; e < b * b; e += SP_NTH) {
                const int i = e % b, j = e / b;
                if (i >= j) {
                    const double cv_ = Cp[sp_at<true>(i, j, ldp)], qv_ = Qp[sp_at<true>(i, j, ldp)];
                    Cg[i + (size_t)j * ldg] = cv_;
                    Qg[i + (size_t)j * ldg] = qv_;
                    if (i > j) {
                        Cg[j + (size_t)i * ldg] = cv_;
                        Qg[j + (size_t)i * ldg] = qv_;
                    }
                }
            }
        } else if (TRI && tri) {
            // the upper triangles from the lower ones: every other kernel (and the full mode) reads full matrices.  16 x 16 tiles, one
            // per 16 lanes and trip, read along their columns (once per call: 16 b^2 bytes against 16 b^2 per POINT)
            const int nt_ = (b + 15) >> 4, sub = tid >> 4, r = tid & 15;
            for (int tl = sub; tl < nt_ * nt_; tl += SP_NTH >> 4) {
                const int ti = tl % nt_, tj = tl / nt_;
                if (ti < tj) continue;
                for (int c = 0; c < 16; ++c) {
                    const int i = 16 * ti + r, j = 16 * tj + c;
                    if (i < b && j < b && i > j) {
                        Cg[j + (size_t)i * ldg] = Cg[i + (size_t)j * ldg];
                        Qg[j + (size_t)i * ldg] = Qg[i + (size_t)j * ldg];
                    }
                }
            }
        }
        if (tid == 0) {
            A.b[patch] = b;
            A.count[patch] += it_end - it0;
            A.stat[patch] = st;
            if (A.status_out) A.status_out[patch] = st;
        }
    }
}

// ---- rows phase: SEVERAL PATCHES PER WAVE -----------------------------------------------------------------------------
// With the reference's default hyper-parameters (src/rbf_kernel.h:24, src/sparse_gp.h:48) a patch keeps about 13 basis vectors
// and 95 % of its points take the projected update (src/sparse_gp.hpp:155-163): one wave per patch leaves 50 of 64 lanes idle
// and the pass is bound by the instruction count of a point's serial skeleton.  Here a patch owns G = 16 (or 32) lanes -- a DPP
// row, where the reductions of a point already live (sp_wave_sum_dpp) -- so a wave carries 4 (2) patches through the same
// instruction stream.  Lane i of a patch holds row i of the basis (k_i, (C k)_i, e_hat_i, alpha_i, BV_i and -- round 4 -- its rows of
// C and Q in registers, in the SLOT layout described below); the B x B blocks in LDS are where a patch is loaded, grown and written
// back; the lanes of different patches diverge only where their branch decisions differ (predication).
// The phase covers what needs no deletion -- first point, projected updates, and full updates that keep the basis within B
// vectors -- and hands a patch over (state written back, points consumed in done_it) BEFORE the first point that needs anything
// else.  Round 4: a second instance (two patches per wave, 24 rows, the listed patches by ticket) continues from there, then the
// one-wave kernel with a resident block of 48 (deletions in place), then the regular kernel; each phase appends what it hands on to
// the next phase's list (gpc_sparse_add_dev).
// A geometric deletion (src/sparse_gp.hpp:226-242) can only follow a full update (the projected update leaves Q alone), and
// whether one would follow is decided from the updated diagonal before anything is written.
// Same operations in the same order per patch as sparse_add_kernel (quarter-wise mat-vec sums, DPP row sums, the next
// point's mat-vecs formed from the updated values): the states are the same bit for bit
// (tests/test_sparse_gpu.py::test_sparse_rows_phase_is_bit_identical).  Gaussian noise only.
template <int G>
__device__ static __forceinline__ double sp_row_sum(double v)
{
    v += sp_dpp<0xB1>(v);      // the four steps of sp_wave_sum_dpp inside the row of 16
    v += sp_dpp<0x4E>(v);
    v += sp_dpp<0x141>(v);
    v += sp_dpp<0x140>(v);
    if (G == 32) v += __shfl_xor(v, 16, 64);           // (row 0 + row 16): the first pair of sp_wave_sum_dpp
    // the absent rows of the one-patch-per-wave layout hold +0.0 terms: (R + 0.0) + (0.0 + 0.0), then the +0.0 of the one-wave shape
    return v + 0.0;
}

// SLOT layout of the rows phase (round 4).  The mat-vec sums of every kernel shape run over four QUARTERS of the columns, quarter q =
// columns [(b q) >> 2, (b (q + 1)) >> 2), each summed in column order -- that is what makes the shapes agree bit for bit.  Indexed by column,
// a lane pays for every slot (q, t) of its row an index, a bound check, a clamp and two addresses: ~7 of the ~10 VALU operations of the
// slot, in a kernel whose time is its VALU count.  So the rows phase keeps C, Q and the vectors k, s, e_hat, k_next by SLOT instead:
// column j of quarter q sits at physical column QN q + (j - start_q), and the slots a quarter does not fill hold +0.0 in every row and
// vector.  A pass is then 16 slots at compile-time addresses with no mask at all: an empty slot computes 0 + x * 0 = +0.0, stores it back
// and adds (+0.0) * (+0.0) to a sum that started at +0.0 -- the same bits as skipping it, as long as x is finite.  The layout moves only
// when the basis grows (columns shift LEFT, never onto a column that has not been read yet if they are taken in column order --
// tests/test_sparse_gpu.py checks the states bit for bit against the other shapes).
template <int QN>
__device__ static __forceinline__ int sp_slot(int j, int b)
{
    const int s1 = b >> 2, s2 = b >> 1, s3 = (3 * b) >> 2;
    const int q = (j >= s1 ? 1 : 0) + (j >= s2 ? 1 : 0) + (j >= s3 ? 1 : 0);
    const int s = q == 0 ? 0 : q == 1 ? s1 : q == 2 ? s2 : s3;
    return QN * q + (j - s);
}

#define SP_FOR_C(c) _Pragma("unroll") for (int c = 0; c < 3; ++c) if (c < ny)   /* static index: the planes stay in registers */
// G lanes per patch, B <= G rows / slots of state (B = G = 16: the first phase, four patches per wave; G = 32, B = 24 = SP_BMAX: the SECOND
// phase, two patches per wave, which takes the patches of the work list -- by ticket -- that the first phase handed over, until they
// outgrow 24 vectors: what the one-wave kernel sparse_add_kernel<true> used to do at ~560 VALU operations per point and patch).
template <int G, int NY, int B = G, bool LIST = false>
__global__ __launch_bounds__(64, 2) void sparse_add_rows_kernel(SpAddParams A)
{
    constexpr int R = 64 / G, QN = B / 4;
    static_assert(B % 4 == 0 && B <= G, "rows of state per patch");
    // A lane keeps its rows of C and Q in REGISTERS between full updates (the passes touch nothing else of the matrices, and
    // every slot index in them is a compile-time value): the update pass reads two vectors from LDS instead of two vectors and two
    // matrices -- 16 KB instead of 40 KB per wave and point through the CU's one LDS pipe, which was as busy as the VALUs.  The LDS
    // blocks stay the place where a patch is loaded, grown (the full update moves columns between slots) and written back; Q in LDS
    // is always current (only the full update writes it), C in LDS only after rows_to_lds().
    // (B == 24, the second phase: 96 registers of rows, and still fewer spilled ones than with the pass's operands in flight -- 176
    // against 256 B of scratch -- and 24 KB instead of 60 KB of LDS traffic per step: 4.90 -> 4.68 ms of add kernels per defaults pass)
    constexpr bool REG = (B == 16 && G == 16) || B == 24;
    constexpr int UNR = (G == 16 || B == 24) ? QN : 2;           // trips of the column loops unrolled together (registers; all of them: slot addresses are immediates)
    constexpr int ROWD = 2 * B * B + 4 * B + (B == G ? 16 : 0);      // doubles of LDS per patch row (+16: de-phases the rows' banks)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* T = reinterpret_cast<double*>(smem);   // 64
    const int lane = threadIdx.x, r = lane / G, i = lane % G;
    double* Cl = T + 64 + r * ROWD;                // C [B slots][B rows]: row i of the column in slot p at i + B p (see sp_slot)
    double* Ql = Cl + B * B;
    double* kvL = Ql + B * B;                      // k of the current point, by slot
    double* svL = kvL + B;                         // s / s_hat
    double* ehL = svL + B;                         // e_hat
    double* knL = ehL + B;                         // k of the next point
    gpc_exp_table_init(T);
    __syncthreads();
    const int ldg = A.ld;
    constexpr int ny = NY;                         // the channel count is a compile-time value here: with a run-time one the compiler
                                                   // evaluates all three channels and selects (6 .. 9 VALU operations per channel loop)
    const double sf = A.prm.sigmaf_sq, s20 = A.prm.noise, eps_tol = A.prm.eps_tol;
    const int capacity = A.prm.capacity;

    for (int base = blockIdx.x * R;; base += gridDim.x * R) {
        int patch;
        bool valid;
        if (LIST) {
            // the patches of the work list, one ticket per group of G lanes (a group that finds the list exhausted idles while the
            // other one works; the wave leaves when every group has)
            // (the first entry of a group is its own index, as in sparse_add_kernel: tickets to one counter are served at ~23 ns each
            // device-wide, and at launch every group asks at once)
            int idx = base + r;
            if (base != (int)blockIdx.x * R) {
                if (i == 0) idx = (int)gridDim.x * R + atomicAdd(A.list_n + A.ticket_slot, 1);
                idx = __shfl(idx, r * G, 64);
            }
            valid = idx < A.list_n[0];
            patch = valid ? A.list[idx] : 0;
            if (!__builtin_amdgcn_ballot_w64(valid)) break;
        } else {
            if (base >= A.P) break;
            patch = base + r;
            valid = patch < A.P;
        }
        const int pc = valid ? patch : A.P - 1;
        const int o = A.off[pc], n = A.off[pc + 1] - o;
        int b = A.b[pc];
        int st = A.stat[pc];
        double* const alphag = A.alpha + (size_t)pc * ny * ldg;
        double* const BVg = A.BV + (size_t)pc * ldg * 2;
        double* const Cg = A.C + (size_t)pc * ldg * ldg;
        double* const Qg = A.Q + (size_t)pc * ldg * ldg;
        const unsigned long long rowmask = ((G == 64) ? ~0ull : ((1ull << G) - 1ull)) << (r * G);   // the lanes of this patch
        const int it0 = A.start_it ? A.start_it[pc] : 0;          // points of this call an earlier phase already took
        bool take = valid && n > 0 && it0 < n && b <= B;
        // state of the patch: rows in registers, blocks in LDS
        double al[3] = {0.0, 0.0, 0.0}, bv0 = 0.0, bv1 = 0.0;
        int ms = (i < b) ? sp_slot<QN>(i, b) : 0;                 // the slot of this lane's own column
        int p00 = b > 0 ? B * sp_slot<QN>(0, b) : 0;              // where C(0, 0) sits
        if (take && i < B) {
            // every slot starts from +0.0 -- rows, columns and vectors; the columns the basis has go to their slots
#pragma unroll
            for (int p = 0; p < B; ++p) {
                Cl[i + B * p] = 0.0;
                Ql[i + B * p] = 0.0;
            }
            kvL[i] = 0.0;
            svL[i] = 0.0;
            ehL[i] = 0.0;
            knL[i] = 0.0;
        }
        if (take && i < b) {
            bv0 = BVg[2 * i];
            bv1 = BVg[2 * i + 1];
            SP_FOR_C(c) al[c] = alphag[c * ldg + i];
            for (int j = 0; j < b; ++j) {
                const int pj = sp_slot<QN>(j, b);
                Cl[i + B * pj] = Cg[i + (size_t)j * ldg];
                Ql[i + B * pj] = Qg[i + (size_t)j * ldg];
            }
        }
        __builtin_amdgcn_wave_barrier();
        double Cr[REG ? B : 1], Qr[REG ? B : 1];
        double c00r = 0.0;                         // REG: C(0, 0) as lane 0 carries it (the NaN check of :245 reads it every point)
#pragma unroll
        for (int p = 0; p < (REG ? B : 1); ++p) { Cr[p] = 0.0; Qr[p] = 0.0; }
        // (lanes beyond the rows of state -- G = 32, B = 24 -- have no row: Cl[i + B p] for i >= B is row i - B of the next slot.  Their loads
        // are harmless and left unmasked -- a masked load keeps the old registers alive and spills the second rows phase -- but their
        // registers must never be stored over it)
        auto rows_to_regs = [&]() {
            if constexpr (REG) {
#pragma unroll
                for (int p = 0; p < B; ++p) {
                    Cr[p] = Cl[i + B * p];
                    Qr[p] = Ql[i + B * p];
                }
                c00r = Cl[p00];
            }
        };
        auto rows_to_lds = [&]() {
            if constexpr (REG) {
                if (B == G || i < B) {
#pragma unroll
                    for (int p = 0; p < B; ++p) Cl[i + B * p] = Cr[p];
                }
            }
        };
        if (take) rows_to_regs();
        {   // a state that already asks for a geometric deletion (possible only for one loaded with gpc_sparse_set_state) is not ours
            const bool asks = take && i < b && b > 1 && (double)1.0f / Ql[i + B * ms] < (double)1e-9f;
            if (__builtin_amdgcn_ballot_w64(asks) & rowmask) take = false;
        }
        if (valid && !take && i == 0) {
            if (LIST) {
                A.done_it[patch] = it0;                             // all of it is the later phases' work
                if (A.out_list && n > 0 && it0 < n) A.out_list[atomicAdd(A.out_list_n, 1)] = patch;
            } else {
                if (!A.start_it) A.done_it[patch] = 0;              // (a later phase leaves the earlier phase's count)
                if (A.list && n > 0 && it0 < n) A.list[atomicAdd(A.list_n, 1)] = patch;   // all of it is the later phases' work
                else if (A.list && A.status_out) A.status_out[patch] = st;                // nothing to do: nobody else visits it
            }
        }
        bool active = take;
        int it = it0, it_end = n;
        bool have_next = false;
        double kn_i = 0.0, pcn[4] = {0.0, 0.0, 0.0, 0.0}, pqn[4] = {0.0, 0.0, 0.0, 0.0};
        // the point in hand, and the next one in flight (two dependent loads: insertion order, then the point)
        double cx0 = 0.0, cx1 = 0.0, cy[3] = {0.0, 0.0, 0.0};
        int r_nxt = 0;
        if (active) {
            const int r0 = A.perm ? A.perm[o + it0] : it0;
            cx0 = A.x0[o + r0];
            cx1 = A.x1[o + r0];
            SP_FOR_C(c) cy[c] = A.y[(size_t)c * A.n_total + o + r0];
            if (it0 + 1 < n) r_nxt = A.perm ? A.perm[o + it0 + 1] : it0 + 1;
        }
        double nx0 = 0.0, nx1 = 0.0, nyv[3] = {0.0, 0.0, 0.0};
        int r_nxt2 = 0;
        // (bottom-tested: with the test at the top the compiler keeps a second copy of every loop-carried value for the exit path and
        // moves ~18 registers there and back per point)
        if (__builtin_amdgcn_ballot_w64(active)) do {
            if (active) {
                const double px0 = cx0, px1 = cx1;
                const double yv[3] = {cy[0], cy[1], cy[2]};
                const bool more = it + 1 < n;
                if (more) {
                    nx0 = A.x0[o + r_nxt];
                    nx1 = A.x1[o + r_nxt];
                    SP_FOR_C(c) nyv[c] = A.y[(size_t)c * A.n_total + o + r_nxt];
                    if (it + 2 < n) r_nxt2 = A.perm ? A.perm[o + it + 2] : it + 2;
                }
                const bool from_prev = have_next;
                have_next = false;
                bool stop = false;                  // hand the patch over before this point
                int dec = 0;
                if (b == 0) {
                    // First point (src/sparse_gp.hpp:100-114)
                    ms = sp_slot<QN>(i, 1);                                  // (meaningful for lane 0)
                    p00 = B * sp_slot<QN>(0, 1);
                    if (i == 0) {
                        const double kstar = sp_kstar(sf, px0, px1);   // kernel_function(X, X)  (:98)
                        SP_FOR_C(c) al[c] = yv[c] / (kstar + s20);
                        Cl[B * ms] = (double)(-1.0f) / (kstar + s20);
                        Ql[B * ms] = (double)(1.0f) / kstar;
                        bv0 = px0;
                        bv1 = px1;
                    }
                    __builtin_amdgcn_wave_barrier();
                    rows_to_regs();
                    b = 1;
                    dec = 0x81;
                } else {
                    // k, C k, e_hat = Q k (:119, :140, :160): from the previous point's update pass, or from scratch
                    // (one set of registers for both: the from-scratch form leaves its k and partial sums where the previous point's pass
                    // leaves them -- eight doubles and k copied per point otherwise)
                    if (!from_prev) {
                        kn_i = 0.0;
                        if (i < b) {
                            kn_i = gpc_rbf_neg(sf, A.c_exp, px0, px1, bv0, bv1, T);
                            kvL[ms] = kn_i;
                        }
                        __builtin_amdgcn_wave_barrier();
                        // the four quarters side by side, one slot of each per trip: their loads are issued together -- QN LDS round trips
                        // per pass instead of one per column; empty slots hold +0.0 (see sp_slot)
                        double acc_[4] = {0.0, 0.0, 0.0, 0.0}, acq_[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll UNR
                        for (int t = 0; t < QN; ++t) {
                            double cv[4], qw[4], kj[4];
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                kj[q] = kvL[QN * q + t];
                                cv[q] = REG ? Cr[REG ? QN * q + t : 0] : Cl[i + B * (QN * q + t)];
                                qw[q] = REG ? Qr[REG ? QN * q + t : 0] : Ql[i + B * (QN * q + t)];
                            }
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                acc_[q] += cv[q] * kj[q];
                                acq_[q] += qw[q] * kj[q];
                            }
                        }
#pragma unroll
                        for (int q = 0; q < 4; ++q) { pcn[q] = acc_[q]; pqn[q] = acq_[q]; }
                    }
                    const double k_i = kn_i;
                    double ck_i = 0.0, eh_i = 0.0;
                    double dots[2] = {0.0, 0.0}, sums[3] = {0.0, 0.0, 0.0};
                    if (i < b) {
                        const double c_ = pcn[0] + pcn[1] + pcn[2] + pcn[3];
                        const double q_ = pqn[0] + pqn[1] + pqn[2] + pqn[3];
                        ck_i = c_;
                        eh_i = q_;
                        dots[0] += k_i * c_;                        // k^T C k   (:122)
                        dots[1] += k_i * q_;                        // k^T e_hat (:144)
                        SP_FOR_C(c) sums[c] += al[c] * k_i;   // m = alpha^T k (:121)
                    }
                    dots[0] = sp_row_sum<G>(dots[0]);
                    dots[1] = sp_row_sum<G>(dots[1]);
                    sums[0] = sp_row_sum<G>(sums[0]);
                    if (ny == 3) {
                        sums[1] = sp_row_sum<G>(sums[1]);
                        sums[2] = sp_row_sum<G>(sums[2]);
                    }
                    const double kstar = sp_kstar(sf, px0, px1);    // kernel_function(X, X)  (:98; formed here: a shorter live range)
                    const double s2 = kstar + dots[0];
                    double gamma = kstar - dots[1];
                    if (gamma < (double)1e-12f) gamma = 0;          // :146-151
                    // gaussian_noise / gaussian_noise_3d (src/gaussian_noise.cpp:9-18, src/gaussian_noise_3d.cpp:11-20)
                    // (the divisions by the same denominator stay the compiler's: sharing the scaled denominator and its refined reciprocal
                    // between them -- 7 of the 13 operations of a division -- was worth 5 % of the colour GP's pass and agreed bit for bit on
                    // every fixed test, but tools/r4_stress_sparse.py found 2 of 300 random configurations, both ill-conditioned with
                    // eps_tol = 1e-14, whose branch decisions then differ from the other kernel shapes': not kept)
                    const double rr = (double)(-1.0f) / (s20 + s2);
                    double qv[3];
                    SP_FOR_C(c) qv[c] = (yv[c] - sums[c]) / (s20 + s2);
                    const bool fuse = A.fuse_next && more;
                    if (gamma < eps_tol && capacity != -1) {
                        // sparse update (:155-163)
                        const double eta = 1 / (1 + gamma * rr);
                        double sh = 0.0;
                        if (i < b) {
                            sh = ck_i + eh_i;                        // s_hat = C*k + e_hat
                            svL[ms] = sh;
                            SP_FOR_C(c) al[c] += sh * (qv[c] * eta);
                        }
                        const double re = rr * eta;
                        if constexpr (REG) c00r = c00r + (re * sh) * sh;          // lane 0: C(0, 0) exactly as the pass below forms it
                        if (fuse && i < b) {
                            kn_i = gpc_rbf_neg(sf, A.c_exp, nx0, nx1, bv0, bv1, T);
                            knL[ms] = kn_i;
                        }
                        __builtin_amdgcn_wave_barrier();
                        {
                            double acc_[4] = {0.0, 0.0, 0.0, 0.0}, acq_[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll UNR
                            for (int t = 0; t < QN; ++t) if (B == G || i < B) {        // (lanes beyond the rows of state have no row)
                                // (no mask: an empty slot is 0 + x * 0 = +0.0 stored back and (+0.0)(+0.0) added to the sums, a row beyond
                                // the basis has s_hat = 0 and stays +0.0; without a next point the sums are never read)
                                double cv[4], qw[4], kj[4], sj[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    sj[q] = svL[QN * q + t];
                                    cv[q] = REG ? Cr[REG ? QN * q + t : 0] : Cl[i + B * (QN * q + t)];
                                    kj[q] = knL[QN * q + t];
                                    qw[q] = REG ? Qr[REG ? QN * q + t : 0] : Ql[i + B * (QN * q + t)];
                                }
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const double c = cv[q] + (re * sh) * sj[q];
                                    if constexpr (REG) Cr[REG ? QN * q + t : 0] = c;
                                    else Cl[i + B * (QN * q + t)] = c;
                                    acc_[q] += c * kj[q];
                                    acq_[q] += qw[q] * kj[q];
                                }
                            }
#pragma unroll
                            for (int q = 0; q < 4; ++q) { pcn[q] = acc_[q]; pqn[q] = acq_[q]; }
                        }
                        have_next = fuse;
                    } else {
                        // full update (:164-203) -- if the basis stays within the block and no deletion follows it
                        const int nb = b + 1;
                        const double ig = (double)1.0f / gamma;
                        const double eh_x = (i < b) ? eh_i : (double)(-1.0f);
                        bool geo = false;
                        if (i < nb) {
                            const double q0 = (i < b) ? Ql[i + B * ms] : 0.0;
                            const double qd = q0 + (ig * eh_x) * eh_x;           // the updated diagonal of Q, as the update forms it
                            geo = (double)1.0f / qd < (double)1e-9f;              // :226-242 would delete
                        }
                        const bool any_geo = (__builtin_amdgcn_ballot_w64(geo) & rowmask) != 0;
                        if (nb > B || nb > ldg || (capacity > 0 && nb > capacity) || any_geo) {
                            stop = true;                    // nothing of this point has been applied
                        } else {
                            dec = 1;
                            rows_to_lds();                                       // (REG: the update and the move between slots happen in LDS)
                            const double si = (i < b) ? ck_i : (double)1.0f;
                            const int msn = sp_slot<QN>(i, nb);                  // this lane's slot in the basis of nb
                            if (i < nb) {
                                svL[msn] = si;
                                ehL[msn] = eh_x;
                                SP_FOR_C(c) {
                                    const double a0 = (i < b) ? al[c] : 0.0;
                                    al[c] = a0 + qv[c] * si;
                                }
                                if (i == b) { bv0 = px0; bv1 = px1; }
                                if (fuse) {
                                    kn_i = gpc_rbf_neg(sf, A.c_exp, nx0, nx1, bv0, bv1, T);
                                    knL[msn] = kn_i;
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            {
                                // The update and the move to the slots of nb columns in one pass, quarter by quarter in COLUMN order: a
                                // column's new slot is never to the right of its old one and never the old slot of a later column, so a
                                // row is rewritten in place (the loads of a quarter precede its stores).  The sums come out in the same
                                // order as everywhere else: quarter q over its columns, ascending.
                                double acc_[4] = {0.0, 0.0, 0.0, 0.0}, acq_[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    const int s0 = (nb * q) >> 2, s1 = (nb * (q + 1)) >> 2;
                                    double cv[QN], qw[QN];
                                    bool ok[QN];
#pragma unroll
                                    for (int t = 0; t < QN; ++t) {
                                        const int j = s0 + t;
                                        ok[t] = j < s1 && i < nb;
                                        const bool old = ok[t] && i < b && j < b;     // the new row / column starts from zero
                                        const int po = old ? sp_slot<QN>(j, b) : 0;
                                        cv[t] = old ? Cl[i + B * po] : 0.0;
                                        qw[t] = old ? Ql[i + B * po] : 0.0;
                                    }
#pragma unroll
                                    for (int t = 0; t < QN; ++t) {
                                        const int pn = QN * q + t;
                                        const double c = cv[t] + (rr * si) * svL[pn];              // (an empty slot: s = e_hat = k = +0.0)
                                        const double qn_ = qw[t] + (ig * eh_x) * ehL[pn];
                                        if (ok[t]) {
                                            Cl[i + B * pn] = c;
                                            Ql[i + B * pn] = qn_;
                                        }
                                        const double kj = knL[pn];
                                        acc_[q] += c * kj;
                                        acq_[q] += qn_ * kj;
                                    }
                                }
#pragma unroll
                                for (int q = 0; q < 4; ++q) { pcn[q] = acc_[q]; pqn[q] = acq_[q]; }
                            }
                            have_next = fuse;
                            b = nb;
                            ms = msn;
                            p00 = B * sp_slot<QN>(0, nb);
                            __builtin_amdgcn_wave_barrier();
                            rows_to_regs();
                        }
                    }
                }
                if (stop) {
                    it_end = it;
                    active = false;
                } else {
                    __builtin_amdgcn_wave_barrier();
                    // isnan(C(0,0)) -> "sparse_gp::C has become Nan" (:245)
                    const double c00 = REG ? c00r : Cl[p00];      // (REG: meaningful in lane 0, which is the one that writes the status)
                    if (c00 != c00 && st == GPC_STATUS_OK) st = GPC_STATUS_NAN;
                    if (A.trace && i == 0) A.trace[o + it] = (uint8_t)dec;
                    ++it;
                    cx0 = nx0; cx1 = nx1; cy[0] = nyv[0]; cy[1] = nyv[1]; cy[2] = nyv[2];
                    r_nxt = r_nxt2;
                    if (it >= n) active = false;
                }
            }
        } while (__builtin_amdgcn_ballot_w64(active));
        // write the state back (a patch handed over continues from it in the next kernel)
        if (take) {
            rows_to_lds();
            __builtin_amdgcn_wave_barrier();
            if (i < b) {
                BVg[2 * i] = bv0;
                BVg[2 * i + 1] = bv1;
                SP_FOR_C(c) alphag[c * ldg + i] = al[c];
                for (int j = 0; j < b; ++j) {
                    const int pj = sp_slot<QN>(j, b);
                    Cg[i + (size_t)j * ldg] = Cl[i + B * pj];
                    Qg[i + (size_t)j * ldg] = Ql[i + B * pj];
                }
            }
            if (i == 0) {
                if (!LIST && A.list && it_end < n) A.list[atomicAdd(A.list_n, 1)] = patch;    // handed over: the next phase continues it
                if (LIST && A.out_list && it_end < n) A.out_list[atomicAdd(A.out_list_n, 1)] = patch;
                A.done_it[patch] = it_end;
                A.b[patch] = b;
                A.count[patch] += it_end - it0;
                A.stat[patch] = st;
                if (A.status_out) A.status_out[patch] = st;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------ host side

static size_t sp_add_lds_small(int bm = SP_BMAX) { return sizeof(double) * (size_t)(64 + 16 + 6 + 4 * (bm + 2) + 22 * (bm + 1) + 2 * bm * bm); }
static size_t sp_add_lds(int ld, bool tri = false) { return sizeof(double) * (size_t)(64 + 16 + 6 + 4 * (ld + 1) + 8 * ld + 9 * ld + 5 * ld + (tri ? 4 * ld : 0)); }

// the rows kernel for the object's ny (1: sparse_gp, 3: sparse_gp_field)
template <int G, int B, bool LIST>
static void sp_rows_launch(const SpAddParams& A, int grid, size_t lds, hipStream_t s)
{
    if (A.ny == 1) hipLaunchKernelGGL((sparse_add_rows_kernel<G, 1, B, LIST>), dim3(grid), dim3(64), lds, s, A);
    else hipLaunchKernelGGL((sparse_add_rows_kernel<G, 3, B, LIST>), dim3(grid), dim3(64), lds, s, A);
}

// capacity <= 64: one wave per patch (every row of the basis fits a lane; no cross-wave barriers, four times the patches
// in flight); capacity <= 100 (the reference's default): two waves, twice the patches in flight; otherwise four waves per
// patch.  While a thread owns at most one basis row the shapes give the same results, bit for bit (GPC_SPARSE_WIDE forces
// the four-wave shape: tests).  Measured at capacity 100: 465 k vs 268 k patches/s in the small-basis regime, 75 k vs 68 k
// with a full basis; at capacity 128 two waves lose (49 k vs 54 k).
int sp_workgroup_threads(const gpc_sparse* g)
{
    const int cap_ = g->prm.capacity;
    return (cap_ <= 0 || getenv("GPC_SPARSE_WIDE")) ? SP_THREADS : cap_ <= 64 ? 64 : cap_ <= 100 ? 128 : SP_THREADS;
}

int sp_add_launch(gpc_sparse* g, const int32_t* off, int n_total, const double* x0, const double* x1, const double* y, const int32_t* perm,
                  int32_t* status)
{
    gpc_ctx* ctx = g->ctx;
    SpAddParams A;
    A.prm = g->prm;
    A.c_exp = (double)(-0.5f) / g->prm.l_sq;
    A.P = g->P; A.ny = g->ny; A.ld = g->ld; A.n_total = n_total;
    A.off = off; A.x0 = x0; A.x1 = x1; A.y = y; A.perm = perm;
    A.alpha = g->alpha; A.C = g->C; A.Q = g->Q; A.BV = g->BV;
    A.b = g->b; A.count = g->count; A.stat = g->stat; A.status_out = status;
    A.fuse_next = getenv("GPC_SPARSE_NO_FUSE") ? 0 : 1;
    A.trace = g->trace;

    const int cap_ = g->prm.capacity, nth0 = sp_workgroup_threads(g);
    // four or two waves per patch (capacity > 64): the triangular mode (sp_tri_pass) -- half the stream of C and Q; GPC_SPARSE_FULL=1 keeps the full passes
    const bool tri = nth0 >= 128 && A.prm.noise_model == GPC_NOISE_GAUSSIAN && !getenv("GPC_SPARSE_FULL");
    // Round 4: 64 < capacity <= 120 (the reference's default is 100, /root/reference/src/sparse_gp.h:48): the lower triangles of C and Q
    // of the patch in flight stay in LDS, packed -- four waves per patch, one patch per CU (sparse_add_kernel<.., RES>; GPC_SPARSE_NO_RES=1
    // keeps the HBM-resident triangular mode of the two-wave shape)
    const size_t lds_res = sp_add_lds(g->ld, true) + sizeof(double) * (size_t)(cap_ + 1) * (size_t)(cap_ + 2);
    // MEASURED AND NOT THE DEFAULT (GPC_SPARSE_RES=1 selects it; 8192 patches x 256 points, basis-filling kernel, same box): capacity 100:
    // 55 k patches/s against 111 k for the HBM-resident two-wave shape, capacity 120: 54 k against 83 k, capacity 80 (two workgroups per
    // CU fit): 125 k against 141 k.  A point costs ~16 us of one workgroup either way (the pass is ~40 instructions per element and the
    // ~20 barrier-separated phases of a point do not overlap inside ONE workgroup), and with the state in LDS a CU hosts one patch where
    // the HBM-resident shape hosts four: the stream it removes was already hidden.  States bit-identical to the HBM-resident mode
    // (tests/test_sparse_gpu.py::test_sparse_lds_resident_mode_is_bit_identical).
    const bool res = tri && cap_ > 64 && lds_res <= 160u * 1024u && getenv("GPC_SPARSE_RES") && !getenv("GPC_SPARSE_NO_RES") && !getenv("GPC_SPARSE_WIDE");
    const int nth = res ? SP_THREADS : nth0;
    const size_t lds = res ? lds_res : sp_add_lds(g->ld, tri);
    A.tri_min = 32;   // (measured at the C4 size: 32 -> 62.0 k patches/s, 96 -> 59.0 k, 160 -> 51.1 k; full passes 42.0 k; the defaults regime is level)
    if (const char* e = getenv("GPC_SPARSE_TRI_MIN")) A.tri_min = atoi(e);      // (diagnostic: where the triangular passes start to pay)
    int per_cu = (int)((160u * 1024u) / lds);
    const int per_cu_max = 2 * SP_THREADS / nth;
    per_cu = per_cu > per_cu_max ? per_cu_max : (per_cu < 1 ? 1 : per_cu);
    int grid = std::min(g->P, ctx->num_cus * per_cu);
    A.start_it = nullptr;
    A.done_it = nullptr;
    A.list = nullptr;
    A.list_n = nullptr;
    A.out_list = nullptr;
    A.out_list_n = nullptr;
    A.ticket_slot = 0;
    const bool gauss = A.prm.noise_model == GPC_NOISE_GAUSSIAN;
    // three work lists in a row, then their counters (4 each): a phase draws from one and appends what it hands on to the next
    int32_t* const L[3] = {g->list, g->list + g->P, g->list + 2 * (size_t)g->P};
    int32_t* const N[3] = {g->list + 3 * (size_t)g->P, g->list + 3 * (size_t)g->P + 4, g->list + 3 * (size_t)g->P + 8};
    int cur = 0;                                   // the list the next phase draws from
    auto hand_on = [&]() { A.out_list = L[cur + 1]; A.out_list_n = N[cur + 1]; };   // the phase in hand appends what it does not finish to the next list
    auto advance = [&]() { ++cur; A.list = L[cur]; A.list_n = N[cur]; A.out_list = A.out_list_n = nullptr; };   // ... which the next phase draws from
    if (!getenv("GPC_SPARSE_NO_SMALL")) {
        // rows phase first (Gaussian noise): four patches per wave while a patch needs at most 16 basis vectors and no deletion;
        // what it does not finish goes on the work list of the phases below
        if (gauss && !getenv("GPC_SPARSE_NO_ROWS")) {
            constexpr int G = 16, R = 64 / G;
            const size_t lds_r = sizeof(double) * (size_t)(64 + R * (2 * G * G + 4 * G + 16));
            A.done_it = g->done_it;
            if (!getenv("GPC_SPARSE_NO_LIST")) {
                A.list = L[0];
                A.list_n = N[0];
                GPC_HIP(ctx, hipMemsetAsync(N[0], 0, 12 * sizeof(int32_t), ctx->stream));
            }
            const int waves = (g->P + R - 1) / R;
            // (a wave per four patches, placed by the hardware as slots come free: patches that leave the phase early end their wave early,
            // and persistent waves striding over the batch carried that imbalance to the end -- 1.93 -> 1.88 ms for the colour GP's pass,
            // level for the depth GP)
            sp_rows_launch<G, G, false>(A, waves, lds_r, ctx->stream);
            GPC_HIP(ctx, hipGetLastError());
            A.start_it = g->done_it;
        }
        // SECOND rows phase (Gaussian noise, round 4): the patches of the list with at most SP_BMAX vectors, two per wave by ticket, until
        // they outgrow SP_BMAX or ask for a deletion, in place of the one-wave kernel below -- a third of that kernel's instructions per
        // point, and a chain of points is as long as the instructions of its steps: 0.36 against 0.51 ms per add call at the reference's
        // defaults (with the first entry of a group taken by index, not by ticket: 4096 tickets at launch were 0.1 ms), bit-identical
        // states.  A patch that asks for a geometric deletion leaves for the mid phase.  GPC_SPARSE_NO_ROWS2=1: the one-wave kernel.
        bool rows2 = false;
        if (gauss && A.list && A.start_it && !getenv("GPC_SPARSE_NO_ROWS2")) {
            constexpr int G2 = 32, B2 = SP_BMAX, R2 = 64 / G2;
            static_assert(B2 == 24, "the second rows phase is built for a resident block of 24");
            const size_t lds_2 = sizeof(double) * (size_t)(64 + R2 * (2 * B2 * B2 + 4 * B2));
            const int per_cu_2 = std::min(8, (int)((160u * 1024u) / lds_2));
            A.ticket_slot = 1;
            hand_on();
            const int waves2 = (g->P + R2 - 1) / R2;
            sp_rows_launch<G2, B2, true>(A, std::min(waves2, ctx->num_cus * per_cu_2), lds_2, ctx->stream);
            GPC_HIP(ctx, hipGetLastError());
            rows2 = true;
            advance();
        }
        // small-basis phase: one wave per patch, C and Q in LDS, until a patch outgrows SP_BMAX basis vectors
        const size_t lds_s = sp_add_lds_small();
        int per_cu_s = (int)((160u * 1024u) / lds_s);
        per_cu_s = per_cu_s > 16 ? 16 : per_cu_s;
        A.done_it = g->done_it;
        A.ticket_slot = 1;
        if (!rows2 && A.list) hand_on();
        if (!gauss)
            hipLaunchKernelGGL((sparse_add_kernel<true, true>), dim3(std::min(g->P, ctx->num_cus * per_cu_s)), dim3(64), lds_s, ctx->stream, A);
        else if (!rows2)
            hipLaunchKernelGGL((sparse_add_kernel<true, false>), dim3(std::min(g->P, ctx->num_cus * per_cu_s)), dim3(64), lds_s, ctx->stream, A);
        GPC_HIP(ctx, hipGetLastError());
        if (!rows2 && A.list) advance();
        A.start_it = g->done_it;
        // mid phase (Gaussian noise, round 4): the patches that have outgrown SP_BMAX vectors -- a few hundred of 32768 at the reference's
        // defaults, each a chain of up to n points -- go through a second instance of the one-wave kernel with a resident block of
        // SP_BMID before the regular kernel sees them: their state in LDS instead of round trips to HBM at every point
        // (GPC_SPARSE_NO_MID=1: straight to the regular kernel)
        if (gauss && A.list && !getenv("GPC_SPARSE_NO_MID") && g->ld > SP_BMAX) {
            const size_t lds_m = sp_add_lds_small(SP_BMID);
            const int per_cu_m = std::max(1, (int)((160u * 1024u) / lds_m));
            A.ticket_slot = 1;
            hand_on();
            hipLaunchKernelGGL((sparse_add_kernel<true, false, false, false, SP_BMID>), dim3(std::min(g->P, ctx->num_cus * per_cu_m)), dim3(64), lds_m,
                               ctx->stream, A);
            GPC_HIP(ctx, hipGetLastError());
            advance();
        }
        A.ticket_slot = 1;
        A.done_it = nullptr;
    }
    if (!gauss) hipLaunchKernelGGL((sparse_add_kernel<false, true>), dim3(grid), dim3(nth), lds, ctx->stream, A);
    else if (res) {
        // per call: the attribute is per device, and a process may hold contexts on several GPUs (idempotent, host-side only)
        GPC_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_add_kernel<false, false, true, true>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        hipLaunchKernelGGL((sparse_add_kernel<false, false, true, true>), dim3(grid), dim3(nth), lds, ctx->stream, A);
    } else if (tri) hipLaunchKernelGGL((sparse_add_kernel<false, false, true>), dim3(grid), dim3(nth), lds, ctx->stream, A);
    else hipLaunchKernelGGL((sparse_add_kernel<false, false>), dim3(grid), dim3(nth), lds, ctx->stream, A);
    GPC_HIP(ctx, hipGetLastError());
    return GPC_OK;
}

