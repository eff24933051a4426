// sparse_device.h -- the device code that the kernels working on the state of the sparse GP share: sparse.hip (the add path) and
// sparse_rate.hip (rate control) include it.  The per-patch state, the block-wide sums and the reference's arg-min, the passes over C and
// Q (full and triangular), delete_bv and its look-ahead.  Everything here is called by all SP_NTH threads of a workgroup.
#pragma once

#include "sparse_internal.h"

struct SpState {
    double *alpha, *C, *Q, *BV;   // this patch
    int ld, ny;                   // ld: stride of the alpha planes (and of the LDS vectors that go with them)
    int ldm;                      // stride of C and Q (== ld in HBM; SP_BMAX when the small-basis kernel keeps them in LDS)
};

// The add kernel and its helpers run with 256 threads per patch, or with 64 (one wave per patch) when capacity <= 64 lets a
// single wave cover every row: SP_NTH is the launch's workgroup size.  Both shapes produce the same bits (the reductions
// and the quarter-wise mat-vec sums are laid out identically); the narrow one has no cross-wave barriers and keeps four
// times as many patches in flight, which is what the small-basis regime needs.
#define SP_NTH ((int)blockDim.x)
#ifndef SP_BMAX
#define SP_BMAX 24   // resident block of the small-basis add kernel (see sparse_add_kernel)
#endif
#define SP_BMID 48   // ... and of its second instance, which takes the patches that have outgrown SP_BMAX (round 4)

// ---- block-wide helpers (all SP_NTH threads call) -------------------------------------------------------

// (every control used here -- quad permutes, row mirrors, row rotate -- has a source lane for every lane, so the destination's previous
// value never shows: the mov form with bound_ctrl spares the `v_mov_b32 dst, 0` that update_dpp(0, ...) puts in front of each of the two
// halves of a double -- 3 instead of 5 VALU operations per step of a row sum, in kernels whose time is their VALU count)
template <int CTRL>
__device__ static __forceinline__ int sp_dpp_i(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
__device__ static __forceinline__ double sp_dpp(double v)
{
    return __hiloint2double(sp_dpp_i<CTRL>(__double2hiint(v)), sp_dpp_i<CTRL>(__double2loint(v)));
}
__device__ static __forceinline__ double sp_readlane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Sum over the 64 lanes of a wave without LDS traffic (the shuffle form costs two ds_bpermute and an LDS round trip per step, six
// steps per sum, eight sums per point: a fifth of the instructions and most of the latency of a point in the small-basis regime).
// Inside a row of 16 the exchanges are symmetric -- quad xor 1, quad xor 2, half-row mirror, row mirror: both partners add the same
// two numbers -- so the 16 lanes of a row end with the same bits; the four row totals then go through SGPRs and are added in one
// fixed order by every lane: the result is uniform by construction (a lane-dependent association would let `gamma < eps_tol`
// diverge inside a wave).
__device__ static __forceinline__ double sp_wave_sum_dpp(double v)
{
    v += sp_dpp<0xB1>(v);      // quad_perm [1,0,3,2]
    v += sp_dpp<0x4E>(v);      // quad_perm [2,3,0,1]
    v += sp_dpp<0x141>(v);     // row_half_mirror
    v += sp_dpp<0x140>(v);     // row_mirror
    return (sp_readlane(v, 0) + sp_readlane(v, 16)) + (sp_readlane(v, 32) + sp_readlane(v, 48));
}

// block-wide sums of the first N (<= 4) entries of v; results broadcast to every thread (the other entries are left alone: a wave
// sum is ~25 instructions, and the callers need 2 + ny of the 8 slots they carry)
template <int N>
__device__ static inline void sp_block_sum4(double (&v)[4], double* scratch /*4*4 doubles*/)
{
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = sp_wave_sum_dpp(v[q]);
    if (SP_NTH == 64) {
        // one-wave shape: what the four-wave layout below computes with three absent waves contributing +0.0 (x + 0.0 is not x for -0.0)
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = ((v[q] + 0.0) + 0.0) + 0.0;
        return;
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < N; ++q) scratch[w * 4 + q] = v[q];
        if (w == 0)                                   // two-wave shape: the absent waves contribute the +0.0 they would have summed
            for (int w2 = SP_NTH >> 6; w2 < 4; ++w2)
#pragma unroll
                for (int q = 0; q < N; ++q) scratch[w2 * 4 + q] = 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) v[q] = scratch[q] + scratch[4 + q] + scratch[8 + q] + scratch[12 + q];
}

// arg-min as the reference scans (src/sparse_gp.hpp:210-217, :229-235: i ascending, `if (i == 0 || score < minscore)`): a NaN score at
// index 0 sticks (every comparison with it is false), a NaN score at any other index is skipped, ties go to the first index.  As a total
// order -- a NaN at index 0 first, then by value with NaN last, then by index -- the winner does not depend on the shape of the reduction;
// rows by DPP, the four row winners through SGPRs.  The scans that feed it use the same order (SP_TAKE(score, i, best, loc)).
#define SP_NAN0(v, i) ((i) == 0 && (v) != (v))
#define SP_TAKE(ov, oi, val, idx) \
    (SP_NAN0(ov, oi) || (!SP_NAN0(val, idx) && ((ov) < (val) || ((ov) == (val) && (oi) < (idx)) || ((val) != (val) && (ov) == (ov)))))
__device__ static inline void sp_block_argmin(double& val, int& idx, double* sval, int* sidx)
{
#define SP_ARGMIN_STEP(CTRL)                                                                                          \
    do {                                                                                                             \
        const double ov = sp_dpp<CTRL>(val);                                                                         \
        const int oi = sp_dpp_i<CTRL>(idx);                                                                          \
        if (SP_TAKE(ov, oi, val, idx)) { val = ov; idx = oi; }                                                       \
    } while (0)
    SP_ARGMIN_STEP(0xB1);
    SP_ARGMIN_STEP(0x4E);
    SP_ARGMIN_STEP(0x141);
    SP_ARGMIN_STEP(0x140);
#undef SP_ARGMIN_STEP
    {
        double bv = sp_readlane(val, 0);
        int bi = __builtin_amdgcn_readlane(idx, 0);
#pragma unroll
        for (int r = 1; r < 4; ++r) {
            const double ov = sp_readlane(val, 16 * r);
            const int oi = __builtin_amdgcn_readlane(idx, 16 * r);
            if (SP_TAKE(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        val = bv;
        idx = bi;
    }
    if (SP_NTH == 64) return;
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sval[w] = val; sidx[w] = idx; }
    __syncthreads();
    val = sval[0];
    idx = sidx[0];
    for (int q = 1; q < SP_NTH / 64; ++q) {
        double ov = sval[q];
        int oi = sidx[q];
        if (SP_TAKE(ov, oi, val, idx)) { val = ov; idx = oi; }
    }
}

// Read-modify-write pass over the nb x nb blocks of C and Q: each thread takes SP_RMW elements per trip, ALL their loads
// first, then the arithmetic and the stores.  Written element by element, a store to C followed by the next load from C
// may alias as far as the compiler can tell, so every iteration waited out a full memory round trip with one load in
// flight per thread (the update was 50-60 % of the time of a point).  f(i, j, c, q) updates the two values in place; the
// element order does not matter (they are independent).
#define SP_RMW 8
template <int RB = SP_RMW, class F>
__device__ static inline void sp_rmw_cq(double* C, double* Q, int ld, int nb, F f)
{
    const int nn = nb * nb;
    for (int e0 = threadIdx.x; e0 < nn; e0 += SP_NTH * RB) {
        double c[RB], q[RB];
        int ii[RB], jj[RB];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            const int e = e0 + u * SP_NTH;
            const int ec = e < nn ? e : e0;                      // clamped: the load is unconditional
            ii[u] = ec % nb;
            jj[u] = ec / nb;
            c[u] = C[ii[u] + (size_t)jj[u] * ld];
            q[u] = Q[ii[u] + (size_t)jj[u] * ld];
        }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            if (e0 + u * SP_NTH < nn) {
                f(ii[u], jj[u], c[u], q[u]);
                C[ii[u] + (size_t)jj[u] * ld] = c[u];
                Q[ii[u] + (size_t)jj[u] * ld] = q[u];
            }
        }
    }
}

// The same pass in the mat-vec's own traversal -- wave w owns the column quarter w, its lanes the rows, columns ascending --
// which lets it hand the NEXT point's mat-vecs C' k' and Q' k' (k' = kvn, evaluated against the basis as it stands after
// this update) out of the values it is about to store: the partial sums land in `pnext` exactly where the stand-alone
// mat-vec of the next iteration would have put them, the same numbers bit for bit, and C and Q are not read a second time
// (a third of the traffic of a point).
#ifndef SP_RMW_NEXT
#define SP_RMW_NEXT 8
#endif
template <bool WRITE_Q = true, int RB = SP_RMW_NEXT, class F>
__device__ static inline void sp_rmw_cq_next(double* C, double* Q, int ld, int lv, int nb, const double* kvn, double* pnext, F f)
{
    const int lane = threadIdx.x & 63;
    if (SP_NTH == 64 && nb <= 32 && (ld == SP_BMAX || ld == SP_BMID)) {     // (ld == SP_BMAX / SP_BMID: C and Q are the LDS blocks of a one-wave kernel)
        // One wave and a small basis (the reference's default hyper-parameters keep it around 13): with a lane per row most of the
        // wave idles and the four column quarters run one after the other -- ~30 instructions per column, 13 columns, every point.
        // Here the lanes form 4 groups of 16 rows (nb <= 16) or 2 groups of 32: group g takes the quarters g, g + G, .. at the same
        // time.  Within a quarter the columns are still visited in ascending order by the lane that owns the row, so every sum
        // is the same sequence of operations as below: the same bits.
        const int shift = nb <= 16 ? 4 : 5;
        const int i = lane & ((1 << shift) - 1), G = 64 >> shift;
        const int cols = (nb + 3) >> 2;                                 // columns of the widest quarter
        for (int quarter = lane >> shift; quarter < 4; quarter += G) {
            const int jlo = (nb * quarter) >> 2, jhi = (nb * (quarter + 1)) >> 2;
            double ac = 0.0, aq = 0.0;
            for (int t = 0; t < cols; ++t) {
                const int j = jlo + t;
                if (j < jhi && i < nb) {
                    double c = C[i + (size_t)j * ld], q = Q[i + (size_t)j * ld];
                    f(i, j, c, q);
                    C[i + (size_t)j * ld] = c;
                    if (WRITE_Q) Q[i + (size_t)j * ld] = q;
                    const double kj = kvn[j];
                    ac += c * kj;
                    aq += q * kj;
                }
            }
            if (i < nb) {
                pnext[(quarter * 2 + 0) * lv + i] = ac;
                pnext[(quarter * 2 + 1) * lv + i] = aq;
            }
        }
        return;
    }
    for (int quarter = threadIdx.x >> 6; quarter < 4; quarter += SP_NTH >> 6) {     // one quarter per wave, or all four in turn
    const int jlo = (nb * quarter) >> 2, jhi = (nb * (quarter + 1)) >> 2;
    for (int i = lane; i < nb; i += 64) {
        double ac = 0.0, aq = 0.0;
        for (int j0 = jlo; j0 < jhi; j0 += RB) {
            double c[RB], q[RB];
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int j = (j0 + u < jhi) ? j0 + u : jhi - 1;      // clamped: the loads are unconditional and come first
                c[u] = C[i + (size_t)j * ld];
                q[u] = Q[i + (size_t)j * ld];
            }
#pragma unroll
            for (int u = 0; u < RB; ++u) {
                const int j = j0 + u;
                if (j < jhi) {
                    f(i, j, c[u], q[u]);
                    C[i + (size_t)j * ld] = c[u];
                    if (WRITE_Q) Q[i + (size_t)j * ld] = q[u];          // the sparse update leaves Q alone: read for Q k' only
                    const double kj = kvn[j];
                    ac += c[u] * kj;
                    aq += q[u] * kj;
                }
            }
        }
        pnext[(quarter * 2 + 0) * lv + i] = ac;
        pnext[(quarter * 2 + 1) * lv + i] = aq;
    }
    }
}

// ---- TRIANGULAR passes (the two- and four-wave shapes of the regular kernel, i.e. capacity > 64, Gaussian noise: SpAddParams::tri) ----------------------------------------
// C and Q are symmetric, and with a large basis the add path is bound by their stream: one read + one write of both per point
// (32 b^2 bytes).  In this mode the kernel works on the LOWER triangles only -- element (i, j), i >= j, at [i + j ld]; the upper
// triangle is ignored on entry and mirrored from the lower one when the patch leaves the kernel, so every other kernel still sees
// full matrices -- 16 b^2 bytes per point.  The element updates are the ones of the full passes, applied to the lower elements
// (same operations, same bits per element from the same inputs); what changes is that a mat-vec takes C_ji for C_ij above the
// diagonal (the full matrices differ from their transposes by a rounding of the rank-one terms) and sums a row in a different
// order: row part (j <= i, in the lane that owns row i) + column part (rows below the diagonal, summed over the lanes).  The
// results are therefore NOT the bits of the full mode (GPC_SPARSE_FULL=1 keeps it: the bit-identity tests between kernel shapes
// run there); they are gated like every other summation order by the parity statistics of tests/sparse_parity.py.
#define SP_TB 8     // columns per block of a triangular pass (8 C + 8 Q column sums = one 16-value wave reduction)
__device__ static __forceinline__ size_t sp_tri_at(int i, int j, int ld)
{
    return i >= j ? (size_t)i + (size_t)j * ld : (size_t)j + (size_t)i * ld;
}
// PACKED lower triangle (round 4: the state of a patch resident in LDS, sparse_add_kernel<.., RES>): column j holds its rows j .. ld - 1
// back to back, so element (i, j), i >= j, sits at  j ld - j (j - 1) / 2 + (i - j);  ld (ld + 1) / 2 doubles per matrix -- 41 KB at the
// reference's default capacity of 100, both matrices in half of a CU's LDS.  PK = false: the strided layout of the state in HBM.
template <bool PK>
__device__ static __forceinline__ size_t sp_at(int i, int j, int ld)        // i >= j
{
    if (PK) return (size_t)(j * ld - ((j * (j - 1)) >> 1) + (i - j));
    return (size_t)i + (size_t)j * ld;
}
template <bool PK>
__device__ static __forceinline__ size_t sp_sym_at(int i, int j, int ld)    // element (i, j) of the symmetric matrix out of its lower triangle
{
    return i >= j ? sp_at<PK>(i, j, ld) : sp_at<PK>(j, i, ld);
}
// first column of wave q's share (of nw = 4, 2 or 1 waves): equal areas of the lower triangle, 1 - sqrt(1 - q / nw), in multiples of SP_TB
__device__ static __forceinline__ int sp_tri_bound(int nb, int q, int nw)
{
    if (q <= 0) return 0;
    if (q >= nw) return nb;
    const double f = nw == 2 ? 0.2928932 : q == 1 ? 0.1339746 : q == 2 ? 0.2928932 : 0.5;
    const int c = ((int)(f * nb + 0.5 * SP_TB)) & ~(SP_TB - 1);
    return c < nb ? c : nb;
}
// Sums the four components of x over the 16 lanes of a DPP row: after the xor-8 and half-mirror rounds a lane keeps ONE component,
// sel = 2 (l >> 3 & 1) + (l >> 2 & 1), which the two quad rounds finish; lanes l & 15 = 0, 4, 8, 12 hold the totals of x0 .. x3.
__device__ static __forceinline__ double sp_row_reduce4(double x0, double x1, double x2, double x3, int r)
{
    const bool hi8 = (r & 8) != 0, hi4 = (r & 4) != 0;
    double k0 = hi8 ? x2 : x0, k1 = hi8 ? x3 : x1;
    const double s0 = hi8 ? x0 : x2, s1 = hi8 ? x1 : x3;
    k0 += sp_dpp<0x128>(s0);            // row_ror:8  (l <-> l ^ 8)
    k1 += sp_dpp<0x128>(s1);
    double k = hi4 ? k1 : k0;
    const double sd = hi4 ? k0 : k1;
    k += sp_dpp<0x141>(sd);             // row_half_mirror
    k += sp_dpp<0xB1>(k);               // quad_perm [1,0,3,2]
    k += sp_dpp<0x4E>(k);               // quad_perm [2,3,0,1]
    return k;
}
// One pass over the lower triangles (256 or 128 threads).  Wave w owns the columns [bound(w), bound(w + 1)); a wave instruction covers
// 16 rows x 4 columns -- lane l: row r = l & 15 of a 16-row group, column g = l >> 4 (and g + 4) of an SP_TB-column block -- so every
// 16-lane segment is one aligned cache line of one column, and the column sums of a block finish inside the DPP rows (no cross-row
// step: 45 instructions per block against 130 for the 16-value wave reduction of the first form, 64 rows x 1 column per instruction).
// A quad's row groups above the diagonal or beyond the basis are issued masked (584 instruction slots per pass at b = 200 for 314
// slots' worth of elements; skipping them behind wave-uniform guards was measured and not kept: the guards end the batch of loads).  Rows OUTSIDE, in quads of row groups, columns inside: the
// row parts of a quad are four register pairs whatever the basis size (with the columns outside they were 2 x 16 accumulators across
// an unrolled body: 110-145 spilled VGPRs), the column parts are reduced per (quad, block) and added up in LDS by the lane that owns
// the column -- the same lane every time, in program order: deterministic.  All 8 + 8 loads of a trip come first.
// MODE bits: 1 apply f(i, j, c, q) and store C | 2 store Q too | 4 mat-vecs with kv: row parts to prow [4][2][lv], column parts
// to pcol [2][lv] | 8 Q is neither read nor written.
template <int MODE, bool PK = false, class F>
__device__ static inline void sp_tri_pass(double* C, double* Q, int ld, int lv, int nb, const double* kv, double* prow, double* pcol, F f)
{
    constexpr bool UPD = (MODE & 1) != 0, WQ = (MODE & 2) != 0, MV = (MODE & 4) != 0, NOQ = (MODE & 8) != 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int nw = SP_NTH >> 6;
    const int jlo = sp_tri_bound(nb, w, nw), jhi = sp_tri_bound(nb, w + 1, nw);
    if (MV) {
        for (int j = jlo + lane; j < jhi; j += 64) pcol[j] = pcol[lv + j] = 0.0;
        if (nw < 4 && w == 0) {                        // two-wave shape: the row parts of the absent waves (the consumer adds four)
            for (int w2 = nw; w2 < 4; ++w2)
                for (int i = lane; i < nb; i += 64) prow[(w2 * 2 + 0) * lv + i] = prow[(w2 * 2 + 1) * lv + i] = 0.0;
        }
    }
    for (int Rq = 0; 16 * Rq < nb; Rq += 4) {
        double rc[4] = {0.0, 0.0, 0.0, 0.0}, rq[4] = {0.0, 0.0, 0.0, 0.0};     // row parts: rows 16 (Rq + t) + r over this lane's columns
        int ic[4];
        double kiv[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 16 * (Rq + t) + r;
            ic[t] = i < nb ? i : nb - 1;
            if (MV) kiv[t] = kv[ic[t]];
        }
        const int jend = jhi < 16 * (Rq + 4) ? jhi : 16 * (Rq + 4);
        for (int j0 = jlo; j0 < jend; j0 += SP_TB) {
            const int ja = j0 + g, jb = j0 + g + 4;
            const bool oka = ja < jhi, okb = jb < jhi;
            const int jac = oka ? ja : jhi - 1, jbc = okb ? jb : jhi - 1;      // clamped: the loads are unconditional
            double ka = 0.0, kb = 0.0;
            if (MV) {
                ka = kv[jac];
                kb = kv[jbc];
            }
            double c[8], q[8];
            int at[8];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    const int jc = s_ ? jbc : jac;
                    at[2 * t + s_] = (int)sp_at<PK>(ic[t] < jc ? jc : ic[t], jc, ld);
                    c[2 * t + s_] = C[at[2 * t + s_]];
                    q[2 * t + s_] = NOQ ? 0.0 : Q[at[2 * t + s_]];
                }
            }
            double cs0 = 0.0, cs1 = 0.0, cq0 = 0.0, cq1 = 0.0;                 // column parts of columns ja, jb: this lane's rows of the quad
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int i = 16 * (Rq + t) + r;
#pragma unroll
                for (int s_ = 0; s_ < 2; ++s_) {
                    const int e = 2 * t + s_, j = s_ ? jb : ja;
                    if ((s_ ? okb : oka) && i >= j && i < nb) {
                        if (UPD) {
                            f(i, j, c[e], q[e]);
                            C[at[e]] = c[e];
                            if (WQ) Q[at[e]] = q[e];
                        }
                        if (MV) {
                            const double kj = s_ ? kb : ka;
                            rc[t] += c[e] * kj;
                            rq[t] += q[e] * kj;
                            if (i > j) {
                                if (s_) { cs1 += c[e] * kiv[t]; cq1 += q[e] * kiv[t]; }
                                else { cs0 += c[e] * kiv[t]; cq0 += q[e] * kiv[t]; }
                            }
                        }
                    }
                }
            }
            if (MV) {
                const double tot = sp_row_reduce4(cs0, cs1, cq0, cq1, r);      // r = 0, 4, 8, 12: C of ja, C of jb, Q of ja, Q of jb
                const int comp = r >> 2, j = (comp & 1) ? jb : ja;
                if ((r & 3) == 0 && j < jhi) pcol[(comp >> 1) * lv + j] += tot;
            }
        }
        if (MV) {
            // a row's four column groups
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                double vc = rc[t], vq = rq[t];
                vc += __shfl_xor(vc, 16, 64);
                vq += __shfl_xor(vq, 16, 64);
                vc += __shfl_xor(vc, 32, 64);
                vq += __shfl_xor(vq, 32, 64);
                const int i = 16 * (Rq + t) + r;
                if (g == 0 && i < nb) {
                    prow[(w * 2 + 0) * lv + i] = vc;
                    prow[(w * 2 + 1) * lv + i] = vq;
                }
            }
        }
    }
}

// delete_bv(loc): sparse_gp.hpp:252-295 / sparse_gp_field.hpp:219-263.  b is workgroup-uniform; returns b-1.
template <int RB, bool TRI = false, bool PK = false>
__device__ static int sp_delete_bv(const SpState& S, int b, int loc, int field_bug, double* Cstar, double* Qstar,
                                   double* Crep, double* Qrep, bool tri_p = false)
{
    const bool tri = TRI && tri_p;      // (this patch runs in the triangular mode)
    const int tid = threadIdx.x, ld = S.ld, ldm = S.ldm, last = b - 1, ny = S.ny;
    double alphastar[3];
    for (int c = 0; c < ny; ++c) alphastar[c] = S.alpha[c * ld + loc];
    const double cstar = S.C[sp_at<PK>(loc, loc, ldm)];
    const double qstar = S.Q[sp_at<PK>(loc, loc, ldm)];
    for (int i = tid; i < b; i += SP_NTH) {
        if (tri) {                                   // columns of the symmetric matrices out of their lower triangles
            const size_t al = sp_sym_at<PK>(i, loc, ldm), aa = sp_sym_at<PK>(last, i, ldm);
            Cstar[i] = S.C[al];
            Qstar[i] = S.Q[al];
            Crep[i] = S.C[aa];
            Qrep[i] = S.Q[aa];
        } else {
            Cstar[i] = S.C[i + (size_t)loc * ldm];
            Qstar[i] = S.Q[i + (size_t)loc * ldm];
            Crep[i] = S.C[i + (size_t)last * ldm];
            Qrep[i] = S.Q[i + (size_t)last * ldm];
        }
    }
    __syncthreads();
    if (tid == 0) {
        Cstar[loc] = Cstar[last];   // Cstar(loc) = Cstar(last)  (:263)
        Qstar[loc] = Qstar[last];   // (:275)
        Crep[loc] = Crep[last];     // (:267)
        Qrep[loc] = Qrep[last];     // (:278)
    }
    __syncthreads();
    for (int i = tid; i < b; i += SP_NTH) {
        const double cr = Crep[i], qr = Qrep[i];
        if (tri) {
            const size_t al = sp_sym_at<PK>(i, loc, ldm);
            S.C[al] = cr;
            S.Q[al] = qr;
        } else {
            S.C[loc + (size_t)i * ldm] = cr;   // C.row(loc) = Crep^T
            S.C[i + (size_t)loc * ldm] = cr;   // C.col(loc) = Crep
            S.Q[loc + (size_t)i * ldm] = qr;
            S.Q[i + (size_t)loc * ldm] = qr;
        }
    }
    if (tid < ny) S.alpha[tid * ld + loc] = S.alpha[tid * ld + last];     // alpha(loc) = alpha(last)  (:257)
    if (tid == 32) {
        S.BV[2 * loc] = S.BV[2 * last];                                     // BV.col(loc) = BV.col(last) (:291)
        S.BV[2 * loc + 1] = S.BV[2 * last + 1];
    }
    __syncthreads();
    const int nb = b - 1;
    const double qc_den = qstar + cstar;
    // alpha update (:285) / field variant (:250-253, multiplies when bug-compatible)
    for (int i = tid; i < nb; i += SP_NTH) {
        const double qc = Qstar[i] + Cstar[i];
        for (int c = 0; c < ny; ++c) {
            if (ny == 1) S.alpha[i] -= alphastar[0] / qc_den * qc;
            else S.alpha[c * ld + i] -= alphastar[c] * (field_bug ? qc_den * qc : qc / qc_den);
        }
    }
    // C += Qs Qs^T / qstar - (Qs+Cs)(Qs+Cs)^T / (qstar+cstar);  Q -= Qs Qs^T / qstar   (:286-288)
    auto downdate = [&](int i, int j, double& c, double& q) {
        const double qq = (Qstar[i] * Qstar[j]) / qstar;
        const double cc = ((Qstar[i] + Cstar[i]) * (Qstar[j] + Cstar[j])) / qc_den;
        c += qq - cc;
        q -= qq;
    };
    if (tri) sp_tri_pass<1 | 2, PK>(S.C, S.Q, ldm, ld, nb, nullptr, nullptr, nullptr, downdate);
    else sp_rmw_cq<RB>(S.C, S.Q, ldm, nb, downdate);
    __syncthreads();
    return nb;
}

// The LOOK-AHEAD of delete_bv(loc): the alpha and BV that sp_delete_bv<.., false, false>(S, b, loc, ..) would leave (b - 1 vectors), into al
// [ny][ld] and bv [ld][2] in LDS -- O(b): column loc of C and Q into Cstar / Qstar, nothing of the O(b^2) downdate, nothing of the state
// written.  A look-ahead instead of remove-and-undo: delete_bv is not invertible in floating point (the downdate of C and Q loses the
// removed row), so an undo would need a copy of the 16 b^2 bytes of state per step, where the look-ahead writes nothing.  The swap
// loc <- last and the alpha update are those of sp_delete_bv above, in its form: the same bits.
__device__ static __forceinline__ void sp_delete_bv_ahead(const SpState& S, int b, int loc, int field_bug, double* Cstar, double* Qstar,
                                                          double* al, double* bv)
{
    const int tid = threadIdx.x, ld = S.ld, last = b - 1, nb = b - 1, ny = S.ny;
    double alphastar[3];
    for (int c = 0; c < ny; ++c) alphastar[c] = S.alpha[c * ld + loc];
    const double cstar = S.C[sp_at<false>(loc, loc, ld)];
    const double qstar = S.Q[sp_at<false>(loc, loc, ld)];
    __syncthreads();                        // (the previous look-ahead's readers of Cstar / Qstar / al / bv are through)
    for (int i = tid; i < b; i += SP_NTH) {
        Cstar[i] = S.C[i + (size_t)loc * ld];
        Qstar[i] = S.Q[i + (size_t)loc * ld];
    }
    __syncthreads();
    if (tid == 0) {
        Cstar[loc] = Cstar[last];
        Qstar[loc] = Qstar[last];
    }
    __syncthreads();
    const double qc_den = qstar + cstar;
    for (int i = tid; i < nb; i += SP_NTH) {
        const int src = i == loc ? last : i;
        const double qc = Qstar[i] + Cstar[i];
        bv[2 * i] = S.BV[2 * src];
        bv[2 * i + 1] = S.BV[2 * src + 1];
        for (int c = 0; c < ny; ++c) {                       // (the loop of sp_delete_bv, in its form)
            double a = S.alpha[c * ld + src];
            if (ny == 1) a -= alphastar[0] / qc_den * qc;
            else a -= alphastar[c] * (field_bug ? qc_den * qc : qc / qc_den);
            al[c * ld + i] = a;
        }
    }
}
