// K5 -- directional potential: matrix-free solve of the fluid-flow system on gfx950.
//
// Reference semantics (paths relative to /root/reference):
//   ssrs/movmodel.py:59-84    assemble_sparse_linear_system: 8-neighbour lists,
//                             sqrt(2) on odd positions of the FILTERED list
//   ssrs/movmodel.py:87-128   solve_sparse_linear_system: conductance
//                             hm(c_i, c_j) (1e-8 if either is 0) / fac, row
//                             normalised G; (I - G_ii) phi_i = G_ib phi_b; spsolve
//   ssrs/movmodel.py:442-447  harmonic_mean
//
// The reference builds the matrix in python loops and factorises it with
// SuperLU (10.8 s at 500x600, infeasible at 5000x6000).  Here nothing is
// assembled: a 9-point variable-coefficient stencil recomputes each row's
// normalised conductances from the conductivity raster on the fly, and the
// system is solved with BiCGStab in f64.  The operator is exactly the
// reference's, including its quirk that east-edge interior nodes weight their
// S neighbour by 1/sqrt(2) and SW by 1 (position parity after filtering).
// Dirichlet cells come from the host (MovModel.get_boundary_nodes restated in
// ssrs_amd/potential.py) as a mask + value raster.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "amg.h"
#include "common.h"

namespace ssrs {

// f32 sqrt(2) widened, as `harmonic_mean(...) / fac` with fac an np.float32
#define SSRS_FAC_DIAG 1.41421353816986083984375

__device__ __forceinline__ double pair_conductance(double a, double b)
{
    return (a != 0.0 && b != 0.0) ? 2.0 / (1.0 / a + 1.0 / b) : 1e-08;
}

// y = (I - G) x on free cells, y = 0 on Dirichlet cells (x is 0 there for
// Krylov vectors; for the residual set-up the caller passes the full field).
// If DOTS: accumulates block partials of (w, y) and (y, y) [w may be NULL -> (x, y)].
struct StencilArgs {
    const double *cond;
    const double *rinv;       // +-1 / cond (0 where cond == 0; sign bit = Dirichlet cell, amg.hip)
                              // when the AMG set it up, else NULL: 2 / (1/a + 1/b) then
                              // costs one division per link, same bits
    const uint8_t *fixed;     // 1 = Dirichlet
    int rows, cols;
    int unnormalised;         // 1: rows of D - C (pairs with the AMG of D - C);
                              // 0: rows of I - G (= Jacobi-scaled, plain Krylov)
    int quirk;                // 1: the reference's east-edge weights (exact operator);
                              // 0: natural weights (symmetric operator, PCG phase)
    TileWalk walk;            // tile order of the stencil kernels (common.h)
};

__device__ __forceinline__ double apply_row(const StencilArgs &a, const double *__restrict__ x,
                                            int r, int c)
{
    const int R = a.rows, C = a.cols;
    const size_t i = static_cast<size_t>(r) * C + c;
    const bool pre = a.rinv != nullptr;
    const double ci = pre ? fabs(a.rinv[i]) : a.cond[i];
    double wsum = 0.0, acc = 0.0;
    const bool east_quirk = a.quirk && (c == C - 1) && r > 0 && r < R - 1;
    // neighbour order is irrelevant for the mathematics; the sum order below is
    // fixed (W, NW, N, NE, E, SE, S, SW) so runs are reproducible
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dr = (k == 1 || k == 2 || k == 3) ? 1 : ((k == 5 || k == 6 || k == 7) ? -1 : 0);
        const int dc = (k == 0 || k == 1 || k == 7) ? -1 : ((k == 3 || k == 4 || k == 5) ? 1 : 0);
        const int rr = r + dr, cc = c + dc;
        if (rr < 0 || rr >= R || cc < 0 || cc >= C) continue;
        bool diag = (dr != 0 && dc != 0);
        if (east_quirk && dr == -1) diag = !diag;     // S <-> SW weights swapped
        const size_t j = static_cast<size_t>(rr) * C + cc;
        double w;
        if (pre) {
            const double rj = fabs(a.rinv[j]);
            w = (ci != 0.0 && rj != 0.0) ? 2.0 / (ci + rj) : 1e-08;
        } else {
            w = pair_conductance(ci, a.cond[j]);
        }
        if (diag) w = w / SSRS_FAC_DIAG;
        wsum += w;
        acc += w * x[j];
    }
    return a.unnormalised ? wsum * x[i] - acc : x[i] - acc / wsum;
}

constexpr int kRedBlocks = 4096;

__device__ __forceinline__ double block_sum(double v, double *lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < kBlock / 64; ++w) s += lds[w];
    __syncthreads();
    return s;   // valid in thread 0
}

// scalars live in device memory so that no iteration waits on the host
struct Scalars {
    double rho, rho_old, alpha, omega, rhat_v, ts, tt, rnorm2, bnorm2, pq, beta;
    double part[6][kRedBlocks];
};

// v = A p ; partial (rhat, v)
__global__ __launch_bounds__(kBlock) void k_apply_dot1(StencilArgs a, const double *__restrict__ p,
                                                      double *__restrict__ v,
                                                      const double *__restrict__ rhat, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d = 0.0;
    for_each_cell(a.walk, [&](size_t i, int r, int c) {
        double y = 0.0;
        if (!a.fixed[i]) y = apply_row(a, p, r, c);
        v[i] = y;
        d += rhat[i] * y;
    });
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[0][blockIdx.x] = d;
}

// s_vec = r - alpha v ; t = A s_vec needs a second pass, so this kernel only forms s_vec
__global__ __launch_bounds__(kBlock) void k_form_s(const double *__restrict__ r,
                                                  const double *__restrict__ v,
                                                  double *__restrict__ sv, size_t n, Scalars *s)
{
    const double alpha = s->alpha;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        sv[i] = r[i] - alpha * v[i];
}

// t = A s_vec ; partials (t, s) and (t, t)
__global__ __launch_bounds__(kBlock) void k_apply_dot2(StencilArgs a, const double *__restrict__ in,
                                                      double *__restrict__ t,
                                                      const double *__restrict__ sv, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d1 = 0.0, d2 = 0.0;
    for_each_cell(a.walk, [&](size_t i, int r, int c) {
        double y = 0.0;
        if (!a.fixed[i]) y = apply_row(a, in, r, c);
        t[i] = y;
        d1 += y * sv[i];
        d2 += y * y;
    });
    d1 = block_sum(d1, lds);
    d2 = block_sum(d2, lds);
    if (threadIdx.x == 0) { s->part[1][blockIdx.x] = d1; s->part[2][blockIdx.x] = d2; }
}

// x += alpha p + omega s ; r = s - omega t ; partials (rhat, r), (r, r)
__global__ __launch_bounds__(kBlock) void k_update_xr(double *__restrict__ x, double *__restrict__ r,
                                                     const double *__restrict__ p,   // M p
                                                     const double *__restrict__ sh,  // M s
                                                     const double *__restrict__ sv,
                                                     const double *__restrict__ t,
                                                     const double *__restrict__ rhat, size_t n,
                                                     Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    const double alpha = s->alpha, omega = s->omega;
    double d1 = 0.0, d2 = 0.0;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        x[i] = x[i] + alpha * p[i] + omega * sh[i];
        const double rn = sv[i] - omega * t[i];
        r[i] = rn;
        d1 += rhat[i] * rn;
        d2 += rn * rn;
    }
    d1 = block_sum(d1, lds);
    d2 = block_sum(d2, lds);
    if (threadIdx.x == 0) { s->part[3][blockIdx.x] = d1; s->part[4][blockIdx.x] = d2; }
}

// p = r + beta (p - omega v)
__global__ __launch_bounds__(kBlock) void k_update_p(double *__restrict__ p,
                                                    const double *__restrict__ r,
                                                    const double *__restrict__ v, size_t n,
                                                    Scalars *s)
{
    const double beta = (s->rho / s->rho_old) * (s->alpha / s->omega);
    const double omega = s->omega;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        p[i] = r[i] + beta * (p[i] - omega * v[i]);
}

// single-block scalar updates between the vector kernels (deterministic sums)
enum { FIN_ALPHA = 0, FIN_OMEGA = 1, FIN_RHO = 2, FIN_INIT = 3, FIN_BNORM = 4, FIN_CG_RHO = 5, FIN_CG_RR = 6, FIN_CG_ALPHA = 7 };
__global__ __launch_bounds__(kBlock) void k_finish(Scalars *s, int what, int nblocks)
{
    __shared__ double lds[kBlock / 64];
    auto total = [&](int slot) {
        double d = 0.0;
        for (int i = threadIdx.x; i < nblocks; i += kBlock) d += s->part[slot][i];
        return block_sum(d, lds);
    };
    if (what == FIN_ALPHA) {
        const double rv = total(0);
        if (threadIdx.x == 0) { s->rhat_v = rv; s->alpha = s->rho / rv; }
    } else if (what == FIN_OMEGA) {
        const double ts = total(1);
        const double tt = total(2);
        if (threadIdx.x == 0) { s->ts = ts; s->tt = tt; s->omega = tt > 0.0 ? ts / tt : 0.0; }
    } else if (what == FIN_RHO) {
        const double rho = total(3);
        const double rr = total(4);
        if (threadIdx.x == 0) { s->rho_old = s->rho; s->rho = rho; s->rnorm2 = rr; }
    } else if (what == FIN_CG_RHO) {         // flexible CG: beta = -(z, q_prev) / (p_prev, q_prev)
        const double zq = total(3);
        if (threadIdx.x == 0) s->beta = s->pq != 0.0 ? -zq / s->pq : 0.0;
    } else if (what == FIN_CG_ALPHA) {       // alpha = (p, r) / (p, q)
        const double pq = total(0);
        const double pr = total(1);
        if (threadIdx.x == 0) { s->pq = pq; s->alpha = pq != 0.0 ? pr / pq : 0.0; }
    } else if (what == FIN_CG_RR) {
        const double rr = total(4);
        if (threadIdx.x == 0) s->rnorm2 = rr;
    } else if (what == FIN_BNORM) {          // |b|^2: residual of the zero field
        const double rr = total(4);
        if (threadIdx.x == 0) s->bnorm2 = rr;
    } else {
        const double rr = total(4);
        if (threadIdx.x == 0) {
            s->rho = rr; s->rho_old = 1.0; s->alpha = 1.0; s->omega = 1.0;
            s->rnorm2 = rr;
        }
    }
}

// ---- preconditioned CG on the symmetric operator (phase 1 of the AMG solve)
__global__ __launch_bounds__(kBlock) void k_cg_dot_rz(const double *__restrict__ r,
                                                     const double *__restrict__ z, size_t n,
                                                     Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d = 0.0;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        d += r[i] * z[i];
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[3][blockIdx.x] = d;
}

__global__ __launch_bounds__(kBlock) void k_cg_p(double *__restrict__ p,
                                                const double *__restrict__ z, size_t n,
                                                Scalars *s, int first)
{
    const double beta = first ? 0.0 : s->beta;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        p[i] = z[i] + beta * p[i];
}

// The same row for one wave = 62 cells of a raster row plus one halo lane on either side
// (needs a.rinv): six loads per lane, the east / west neighbours by lane shuffles.  The
// thread-per-cell form is bound by its 17 load instructions per cell, not by bytes
// (0.79 -> 0.5 ms per application at 5000 x 6000).  Same operation order, same bits.
constexpr int kWaveCols = 62;
__device__ __forceinline__ double apply_row_wave(const StencilArgs &a, const double *__restrict__ x, int r,
                                                 int c, bool &centre, bool &fixed, size_t &i, double &xi)
{
    const int R = a.rows, C = a.cols, lane = threadIdx.x & 63;
    const bool col_ok = c >= 0 && c < C;
    double xv[3], sv[3];                                      // rows r-1, r, r+1 of this lane's column
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const int rr = r + d - 1;
        const bool ok = col_ok && rr >= 0 && rr < R;
        const size_t j = static_cast<size_t>(ok ? rr : r) * C + (col_ok ? c : 0);
        xv[d] = ok ? x[j] : 0.0;
        sv[d] = ok ? a.rinv[j] : __builtin_inf();             // +inf: outside the raster, no link
    }
    i = static_cast<size_t>(r) * C + (col_ok ? c : 0);
    centre = col_ok && lane >= 1 && lane <= kWaveCols;
    fixed = signbit(sv[1]);
    xi = xv[1];
    const double ci = fabs(sv[1]);
    double wsum = 0.0, acc = 0.0;
    const bool east_quirk = a.quirk && (c == C - 1) && r > 0 && r < R - 1;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                             // W, NW, N, NE, E, SE, S, SW as in apply_row
        const int dr = (k == 1 || k == 2 || k == 3) ? 1 : ((k == 5 || k == 6 || k == 7) ? -1 : 0);
        const int dc = (k == 0 || k == 1 || k == 7) ? -1 : ((k == 3 || k == 4 || k == 5) ? 1 : 0);
        double sj = sv[dr + 1], xj = xv[dr + 1];
        if (dc < 0) { sj = __shfl_up(sj, 1); xj = __shfl_up(xj, 1); }
        if (dc > 0) { sj = __shfl_down(sj, 1); xj = __shfl_down(xj, 1); }
        const double rj = fabs(sj);
        bool diag = (dr != 0 && dc != 0);
        if (east_quirk && dr == -1) diag = !diag;             // S <-> SW weights swapped
        double w = (ci != 0.0 && rj != 0.0) ? 2.0 / (ci + rj) : 1e-08;
        if (diag) w = w / SSRS_FAC_DIAG;
        if (rj == __builtin_inf()) w = 0.0;                   // (adds exact zeros: same sums as skipping)
        wsum += w;
        acc += w * xj;
    }
    return a.unnormalised ? wsum * xv[1] - acc : xv[1] - acc / wsum;
}

__global__ __launch_bounds__(kBlock) void k_cg_apply_wave(StencilArgs a, const double *__restrict__ p,
                                                         double *__restrict__ q,
                                                         const double *__restrict__ r, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    const int per_block = (kBlock / 64) * kWaveCols;
    const int segs = (a.cols + per_block - 1) / per_block;
    const long long items = static_cast<long long>(a.rows) * segs;
    double d0 = 0.0, d1 = 0.0;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int row = static_cast<int>(it / segs), seg = static_cast<int>(it - static_cast<long long>(row) * segs);
        const int c = (seg * (kBlock / 64) + static_cast<int>(threadIdx.x >> 6)) * kWaveCols +
                      static_cast<int>(threadIdx.x & 63) - 1;
        bool centre, fixed;
        size_t i;
        double pi;
        double y = apply_row_wave(a, p, row, c, centre, fixed, i, pi);
        if (centre) {
            if (fixed) y = 0.0;
            q[i] = y;
            d0 += pi * y;
            d1 += pi * r[i];
        }
    }
    d0 = block_sum(d0, lds);
    d1 = block_sum(d1, lds);
    if (threadIdx.x == 0) { s->part[0][blockIdx.x] = d0; s->part[1][blockIdx.x] = d1; }
}

// wave forms of k_apply_dot1 / k_apply_dot2 (BiCGStab polish on the exact operator)
__global__ __launch_bounds__(kBlock) void k_apply_dot1_wave(StencilArgs a, const double *__restrict__ p,
                                                           double *__restrict__ v,
                                                           const double *__restrict__ rhat, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    const int per_block = (kBlock / 64) * kWaveCols;
    const int segs = (a.cols + per_block - 1) / per_block;
    const long long items = static_cast<long long>(a.rows) * segs;
    double d = 0.0;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int row = static_cast<int>(it / segs), seg = static_cast<int>(it - static_cast<long long>(row) * segs);
        const int c = (seg * (kBlock / 64) + static_cast<int>(threadIdx.x >> 6)) * kWaveCols +
                      static_cast<int>(threadIdx.x & 63) - 1;
        bool centre, fixed;
        size_t i;
        double pi;
        double y = apply_row_wave(a, p, row, c, centre, fixed, i, pi);
        if (centre) {
            if (fixed) y = 0.0;
            v[i] = y;
            d += rhat[i] * y;
        }
    }
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[0][blockIdx.x] = d;
}

__global__ __launch_bounds__(kBlock) void k_apply_dot2_wave(StencilArgs a, const double *__restrict__ in,
                                                           double *__restrict__ t,
                                                           const double *__restrict__ sv, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    const int per_block = (kBlock / 64) * kWaveCols;
    const int segs = (a.cols + per_block - 1) / per_block;
    const long long items = static_cast<long long>(a.rows) * segs;
    double d1 = 0.0, d2 = 0.0;
    for (long long it = blockIdx.x; it < items; it += gridDim.x) {
        const int row = static_cast<int>(it / segs), seg = static_cast<int>(it - static_cast<long long>(row) * segs);
        const int c = (seg * (kBlock / 64) + static_cast<int>(threadIdx.x >> 6)) * kWaveCols +
                      static_cast<int>(threadIdx.x & 63) - 1;
        bool centre, fixed;
        size_t i;
        double xi;
        double y = apply_row_wave(a, in, row, c, centre, fixed, i, xi);
        if (centre) {
            if (fixed) y = 0.0;
            t[i] = y;
            d1 += y * sv[i];
            d2 += y * y;
        }
    }
    d1 = block_sum(d1, lds);
    d2 = block_sum(d2, lds);
    if (threadIdx.x == 0) { s->part[1][blockIdx.x] = d1; s->part[2][blockIdx.x] = d2; }
}

// q = A p ; partials (p, q) and (p, r)
__global__ __launch_bounds__(kBlock) void k_cg_apply(StencilArgs a, const double *__restrict__ p,
                                                    double *__restrict__ q,
                                                    const double *__restrict__ r, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d0 = 0.0, d1 = 0.0;
    for_each_cell(a.walk, [&](size_t i, int rr, int cc) {
        double y = 0.0;
        if (!a.fixed[i]) y = apply_row(a, p, rr, cc);
        q[i] = y;
        d0 += p[i] * y;
        d1 += p[i] * r[i];
    });
    d0 = block_sum(d0, lds);
    d1 = block_sum(d1, lds);
    if (threadIdx.x == 0) { s->part[0][blockIdx.x] = d0; s->part[1][blockIdx.x] = d1; }
}

__global__ __launch_bounds__(kBlock) void k_cg_xr(double *__restrict__ x, double *__restrict__ r,
                                                 const double *__restrict__ p,
                                                 const double *__restrict__ q, size_t n, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    const double alpha = s->alpha;
    double d = 0.0;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        x[i] = x[i] + alpha * p[i];
        const double rn = r[i] - alpha * q[i];
        r[i] = rn;
        d += rn * rn;
    }
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[4][blockIdx.x] = d;
}

// ---- the east-edge quirk as a defect of the symmetric operator (phase 2 of the AMG solve).
// The exact operator A_q differs from the symmetric one A_s in the rows of the east-edge interior cells only: their S link
// is weighted as a diagonal one (/ sqrt 2) and their SW link as a straight one (movmodel.py:75-79, position parity in the
// FILTERED neighbour list).  In the D - C form of a row
//     (A_q x - A_s x)_i = (w_S / f - w_S) (x_i - x_S) + (w_SW - w_SW / f) (x_i - x_SW),      f = sqrt 2 as f32,
// a few thousand numbers formed from DIFFERENCES of neighbouring potentials -- no cancellation, unlike a recomputed
// residual (whose rounding noise is ~3e-6 |b| at 5000 x 6000).  r = b - A_q x is kept up to date by
//     r_i -= E_i(x) - E_i(x at the previous update),
// after which the SAME preconditioned CG on A_s goes on from the corrected residual (directions restarted).  Nothing in
// it can stagnate or break down the way BiCGStab does (soak case 342679122: restarts exhausted at 2.4e-14, the field
// 2.6e-2 off; with this: 420 iterations, 6.5e-4), but an update only shrinks the defect by the contraction factor of
// A_s^-1 E, ~0.1 at 5000 x 6000 -- eleven rounds and 1 460 iterations where BiCGStab takes 130 -- so it is the FALL-BACK:
// BiCGStab first, and only a solve that BiCGStab leaves unconverged goes back to PCG's iterate and through this.
__global__ __launch_bounds__(kBlock) void k_quirk_defect(StencilArgs a, const double *__restrict__ x,
                                                        double *__restrict__ e_prev, double *__restrict__ r)
{
    const int R = a.rows, C = a.cols;
    for (int row = blockIdx.x * kBlock + threadIdx.x; row < R; row += gridDim.x * kBlock) {
        double e = 0.0;
        const size_t i = static_cast<size_t>(row) * C + (C - 1);
        if (row > 0 && row < R - 1 && C >= 2 && !a.fixed[i]) {
            const size_t js = i - C, jsw = i - C - 1;
            double ws, wsw;
            if (a.rinv) {
                const double ci = fabs(a.rinv[i]), rs = fabs(a.rinv[js]), rsw = fabs(a.rinv[jsw]);
                ws = (ci != 0.0 && rs != 0.0) ? 2.0 / (ci + rs) : 1e-08;
                wsw = (ci != 0.0 && rsw != 0.0) ? 2.0 / (ci + rsw) : 1e-08;
            } else {
                ws = pair_conductance(a.cond[i], a.cond[js]);
                wsw = pair_conductance(a.cond[i], a.cond[jsw]);
            }
            e = (ws / SSRS_FAC_DIAG - ws) * (x[i] - x[js]) + (wsw - wsw / SSRS_FAC_DIAG) * (x[i] - x[jsw]);
            r[i] -= e - e_prev[row];
        }
        e_prev[row] = e;
    }
}

__global__ __launch_bounds__(kBlock) void k_norm2(const double *__restrict__ r, size_t n, Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d = 0.0;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock)
        d += r[i] * r[i];
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[4][blockIdx.x] = d;
}

// set-up: x0 = Dirichlet values on fixed cells / initial guess elsewhere;
// r = b - A x0 (b = 0 on free cells), rhat = r, p = r, v = 0; partial (r, r)
__global__ __launch_bounds__(kBlock) void k_setup(StencilArgs a, const double *__restrict__ x,
                                                 double *__restrict__ r, double *__restrict__ rhat,
                                                 double *__restrict__ p, double *__restrict__ v,
                                                 Scalars *s)
{
    __shared__ double lds[kBlock / 64];
    double d = 0.0;
    for_each_cell(a.walk, [&](size_t i, int rr, int cc) {
        double res = 0.0;
        if (!a.fixed[i]) res = -apply_row(a, x, rr, cc);
        r[i] = res; rhat[i] = res; p[i] = res; v[i] = 0.0;
        d += res * res;
    });
    d = block_sum(d, lds);
    if (threadIdx.x == 0) s->part[4][blockIdx.x] = d;
}

// diagnostics (SSRS_PROGRESS): where a recomputed residual sits -- sums of r^2 over live cells (cond != 0), dead cells
// and the east-edge column, the largest |r| and its cell
__global__ __launch_bounds__(kBlock) void k_resid_breakdown(StencilArgs a, const double *__restrict__ r, double *__restrict__ out)
{
    const size_t n = static_cast<size_t>(a.rows) * a.cols;
    double live = 0.0, dead = 0.0, east = 0.0, big = 0.0;
    unsigned long long where = 0;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * kBlock) {
        const double v = r[i];
        const bool is_dead = a.rinv ? a.rinv[i] == 0.0 : a.cond[i] == 0.0;
        if (static_cast<int>(i % a.cols) == a.cols - 1) east += v * v;
        else if (is_dead) dead += v * v;
        else live += v * v;
        if (fabs(v) > big) { big = fabs(v); where = i; }
    }
    atomicAdd(&out[0], live); atomicAdd(&out[1], dead); atomicAdd(&out[2], east);
    // (max by the bit pattern of a non-negative double; the cell of the last writer that held the maximum)
    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(big));
    if (atomicMax(reinterpret_cast<unsigned long long *>(&out[3]), bits) < bits) reinterpret_cast<unsigned long long *>(out)[4] = where;
}

__global__ __launch_bounds__(kBlock) void k_init_x(const uint8_t *__restrict__ fixed,
                                                  const double *__restrict__ fixed_val,
                                                  const double *__restrict__ guess, double fill,
                                                  double *__restrict__ x, int rows, int cols)
{
    const size_t n = static_cast<size_t>(rows) * cols;
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        x[i] = fixed[i] ? fixed_val[i] : (guess ? guess[i] : fill);
}

__global__ __launch_bounds__(kBlock) void k_to_f32(const double *__restrict__ x,
                                                  float *__restrict__ out, size_t n)
{
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock)
        out[i] = static_cast<float>(x[i]);
}

// The range of the Dirichlet values, one block: range[0] = min, range[1] = max (min > max: no Dirichlet cell).  The
// rows of the operator are convex combinations (positive weights, normalised), so the solution lies in this range.
__global__ __launch_bounds__(kBlock) void k_dirichlet_range(const uint8_t *__restrict__ fixed,
                                                           const double *__restrict__ fixed_val, size_t n,
                                                           double *__restrict__ range)
{
    __shared__ double lds[2][kBlock / 64];
    double lo = __builtin_inf(), hi = -__builtin_inf();
    for (size_t i = threadIdx.x; i < n; i += kBlock)
        if (fixed[i]) { lo = fmin(lo, fixed_val[i]); hi = fmax(hi, fixed_val[i]); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { lo = fmin(lo, __shfl_down(lo, off)); hi = fmax(hi, __shfl_down(hi, off)); }
    if ((threadIdx.x & 63) == 0) { lds[0][threadIdx.x >> 6] = lo; lds[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) { lo = fmin(lo, lds[0][w]); hi = fmax(hi, lds[1][w]); }
        range[0] = lo;
        range[1] = hi;
    }
}

// An iterate that did not converge need not obey the maximum principle: projected onto the range of the Dirichlet
// values, which holds the solution, it is nowhere further from it than before
__global__ __launch_bounds__(kBlock) void k_to_f32_clamped(const double *__restrict__ x, float *__restrict__ out, size_t n,
                                                          const double *__restrict__ range)
{
    const double lo = range[0], hi = range[1];
    for (size_t i = blockIdx.x * static_cast<size_t>(kBlock) + threadIdx.x; i < n;
         i += static_cast<size_t>(gridDim.x) * kBlock) {
        const double xi = x[i];
        out[i] = static_cast<float>(lo <= hi && xi == xi ? fmin(fmax(xi, lo), hi) : xi);     // (a NaN stays visible)
    }
}

static size_t vec_bytes(size_t n) { return (n * 8 + 255) / 256 * 256; }

// The solver's switches from the environment, read at the start of every call (tests set them between calls)
struct SolverSwitches {
    bool progress;               // SSRS_PROGRESS: heartbeat, carried against recomputed residuals on stderr
    bool progress_every;         // SSRS_PROGRESS=2: a line at every check
    bool fallback;               // off if SSRS_SOLVE_NO_FALLBACK: BiCGStab's answer as it is, no defect correction
    bool blocks0, fuse;          // off if SSRS_AMG_NO_BLOCKS, SSRS_AMG_NO_FUSE (amg.h)
    int nu0, nuc;                // SSRS_AMG_NU=a,b (amg.h)
};

static SolverSwitches read_solver_switches()
{
    auto set = [](const char *name) { return std::getenv(name) != nullptr; };
    SolverSwitches sw;
    const char *progress = std::getenv("SSRS_PROGRESS");
    sw.progress = progress != nullptr;
    sw.progress_every = progress != nullptr && std::atoi(progress) >= 2;
    sw.fallback = !set("SSRS_SOLVE_NO_FALLBACK");
    sw.blocks0 = !set("SSRS_AMG_NO_BLOCKS");
    sw.fuse = !set("SSRS_AMG_NO_FUSE");
    sw.nu0 = sw.nuc = 1;
    if (const char *e = std::getenv("SSRS_AMG_NU")) {
        int a0 = 2, a1 = 2;
        if (std::sscanf(e, "%d,%d", &a0, &a1) == 2) { sw.nu0 = a0 == 1 ? 1 : 2; sw.nuc = a1 == 1 ? 1 : 2; }
    }
    return sw;
}

// The events of a call, released on every way out of it
struct SolveEvents {
    hipEvent_t setup0 = nullptr, setup1 = nullptr;   // around the AMG set-up
    hipEvent_t first = nullptr, last = nullptr;      // around the iteration
    SolveEvents() = default;
    SolveEvents(const SolveEvents &) = delete;
    SolveEvents &operator=(const SolveEvents &) = delete;
    ~SolveEvents()
    {
        for (hipEvent_t e : {setup0, setup1, first, last})
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace ssrs

using namespace ssrs;

extern "C" size_t ssrs_potential_workspace_bytes(int rows, int cols)
{
    if (rows <= 0 || cols <= 0) return 0;
    const size_t n = static_cast<size_t>(rows) * cols;
    return (sizeof(Scalars) + 255) / 256 * 256 + 11 * vec_bytes(n) + amg_workspace_bytes(rows, cols) + 256;
}

typedef struct SsrsSolveStatsInternal {
    int32_t iterations, converged;
    double residual;
    float kernel_ms;
    int32_t amg_levels, amg_coarsest;
    float setup_ms;
    uint64_t workspace_used;
} SsrsSolveStatsInternal;
static_assert(sizeof(SsrsSolveStatsInternal) == sizeof(SsrsSolveStats), "stats layout");

namespace {

// One call of ssrs_potential_solve: the workspace's vectors, the hierarchy and the state the phases hand on
struct SolveRun {
    const double *cond, *fixed_values, *guess;
    const uint8_t *fixed;
    float *potential;
    int rows, cols;
    double rel_tol;
    int max_iterations;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t st;
    const SolverSwitches sw;
    SolveEvents ev;
    const size_t n;
    Scalars *sc;
    char *base;                            // the solver's vectors, then the hierarchy's workspace
    double *x, *r, *rhat, *p, *v, *sv, *t;
    double *xbest, *phat, *shat;
    double *x_pcg;                         // PCG's iterate, kept for the fall-back of phase 2
    // right-preconditioned BiCGStab: M = one AMG V-cycle of the symmetric operator
    const bool use_amg;
    AmgHierarchy amg;
    float setup_ms = 0.f;
    size_t ws_used;
    StencilArgs a = {}, as = {};           // the exact operator; the symmetric one (natural weights)
    int nb = 0;
    double host[2] = {0.0, 0.0};
    // PCG
    int cg_iterations = 0;
    bool restart_dirs = true;
    bool pcg_ok = false;                   // PCG reached rel_tol on the symmetric operator
    // BiCGStab
    int it = 0, converged = 0, robust_from = -1;
    double rel = 1.0, best = 1e300;

    SolveRun(const double *conductivity, const uint8_t *fixed_mask, const double *fixed_vals, const double *initial_guess,
             float *pot, int rows_, int cols_, double tol, int max_it, int flags, void *ws, size_t ws_bytes, hipStream_t stream)
        : cond(conductivity), fixed_values(fixed_vals), guess(initial_guess), fixed(fixed_mask), potential(pot),
          rows(rows_), cols(cols_), rel_tol(tol), max_iterations(max_it), workspace(ws), workspace_bytes(ws_bytes), st(stream),
          sw(read_solver_switches()), n(static_cast<size_t>(rows_) * cols_), use_amg((flags & SSRS_SOLVE_NO_AMG) == 0)
    {
        base = static_cast<char *>(workspace);
        sc = reinterpret_cast<Scalars *>(base);
        base += (sizeof(Scalars) + 255) / 256 * 256;
        double *vec[11];
        for (int i = 0; i < 11; ++i) vec[i] = reinterpret_cast<double *>(base + i * vec_bytes(n));
        x = vec[0]; r = vec[1]; rhat = vec[2]; p = vec[3]; v = vec[4]; sv = vec[5]; t = vec[6];
        xbest = vec[7]; phat = vec[8]; shat = vec[9]; x_pcg = vec[10];
        amg.sweeps = 1 + ((flags >> 4) & 7);
        amg.nu0 = sw.nu0;
        amg.nuc = sw.nuc;
        amg.blocks0 = sw.blocks0;
        amg.fuse = sw.fuse;
        amg.progress = sw.progress;
        amg.kdepth = (flags & SSRS_SOLVE_K_CYCLE) ? (((flags >> 12) & 15) ? ((flags >> 12) & 15) : 3) : 0;
        amg.symmetric = (flags & SSRS_SOLVE_ONE_SIDED) == 0;
        amg.strong_rounds = ((flags >> 8) & 15) ? ((flags >> 8) & 15) : 4;
        ws_used = static_cast<size_t>(11 * vec_bytes(n)) + 512;
    }
    ~SolveRun() { amg_release(amg); }      // the captured graph is host state: freed on every exit
    SolveRun(const SolveRun &) = delete;
    SolveRun &operator=(const SolveRun &) = delete;

    int setup_amg();
    int start();
    int pcg(double tol, int cap, double &reached);
    int pcg_phase();
    int report_pcg();
    int bicgstab();
    int fall_back();
    int finish(void *stats_out);
};

// The hierarchy, in the workspace behind the solver's vectors
int SolveRun::setup_amg()
{
    SSRS_HIP_CHECK(hipEventCreate(&ev.setup0));
    SSRS_HIP_CHECK(hipEventCreate(&ev.setup1));
    SSRS_HIP_CHECK(hipEventRecord(ev.setup0, st));
    char *amg_base = base + 11 * vec_bytes(n);
    amg_base = reinterpret_cast<char *>((reinterpret_cast<uintptr_t>(amg_base) + 255) / 256 * 256);
    const size_t amg_bytes = static_cast<size_t>(static_cast<char *>(workspace) + workspace_bytes - amg_base);
    const int rc = amg_setup(amg, cond, fixed, rows, cols, amg_base, amg_bytes, st);
    (void)hipEventRecord(ev.setup1, st);
    (void)hipEventSynchronize(ev.setup1);
    (void)hipEventElapsedTime(&setup_ms, ev.setup0, ev.setup1);
    if (rc != SSRS_OK) return rc;
    ws_used += amg.workspace_used;
    return SSRS_OK;
}

// |b| (the stopping criterion is |r| <= rel_tol |b|, independent of the start) and the start field with its residual
int SolveRun::start()
{
    a = StencilArgs{cond, use_amg ? amg.l0_rinv : nullptr, fixed, rows, cols, use_amg ? 1 : 0, 1, make_tile_walk(rows, cols)};
    as = a;
    as.quirk = 0;
    nb = static_cast<int>((n + kBlock - 1) / kBlock);
    if (nb > kRedBlocks) nb = kRedBlocks;
    SSRS_HIP_CHECK(hipEventCreate(&ev.first));
    SSRS_HIP_CHECK(hipEventCreate(&ev.last));
    SSRS_HIP_CHECK(hipEventRecord(ev.first, st));
    SSRS_HIP_CHECK(hipMemsetAsync(sc, 0, sizeof(Scalars), st));
    hipLaunchKernelGGL(k_init_x, dim3(nb), dim3(kBlock), 0, st, fixed, fixed_values,
                       static_cast<const double *>(nullptr), 0.0, x, rows, cols);
    hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, a, x, r, rhat, p, v, sc);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_BNORM, nb);
    // start field: caller's guess, else the mid value 500
    hipLaunchKernelGGL(k_init_x, dim3(nb), dim3(kBlock), 0, st, fixed, fixed_values, guess, 500.0, x, rows, cols);
    hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, a, x, r, rhat, p, v, sc);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// Preconditioned (flexible) CG on the symmetric operator A_s from the carried residual r, until |r| <= tol |b| or
// cg_iterations reaches `cap`; `reached` = the last |r| / |b| it saw.  Phase 1 of the AMG solve, and the engine of
// phase 2's fall-back.
int SolveRun::pcg(double tol, int cap, double &reached)
{
    double cg_best = 1e300, now = 1e300;
    int stalled = 0;
    while (cg_iterations < cap) {
        for (int j = 0; j < 5; ++j, ++cg_iterations) {
            // flexible CG(1): p is A-orthogonalised explicitly against the previous direction
            amg_apply(amg, r, phat, st);                                                         // z = M r
            hipLaunchKernelGGL(k_cg_dot_rz, dim3(nb), dim3(kBlock), 0, st, phat, v, n, sc);      // (z, q_prev)
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_CG_RHO, nb);
            hipLaunchKernelGGL(k_cg_p, dim3(nb), dim3(kBlock), 0, st, p, phat, n, sc, restart_dirs ? 1 : 0);
            restart_dirs = false;
            if (as.rinv)                                                                         // q = A p
                hipLaunchKernelGGL(k_cg_apply_wave, dim3(nb), dim3(kBlock), 0, st, as, p, v, r, sc);
            else
                hipLaunchKernelGGL(k_cg_apply, dim3(nb), dim3(kBlock), 0, st, as, p, v, r, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_CG_ALPHA, nb);
            hipLaunchKernelGGL(k_cg_xr, dim3(nb), dim3(kBlock), 0, st, x, r, p, v, n, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_CG_RR, nb);
        }
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(host, &sc->rnorm2, 2 * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess) return SSRS_ERR_HIP;
        if (!(host[0] == host[0])) break;
        now = host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : 0.0;
        if (sw.progress && (cg_iterations % 250 == 0 || sw.progress_every))
            fprintf(stderr, "[ssrs_potential_solve] PCG it %d |r|/|b| %.3e\n", cg_iterations, now);
        if (now <= tol) break;
        if (now < 0.9 * cg_best) { cg_best = now; stalled = 0; }
        else if (++stalled >= 100) break;          // 500 iterations without a 10 % gain
    }
    reached = now;
    return SSRS_OK;
}

// ---- phase 1: PCG on the symmetric operator (natural weights).  One V-cycle + one operator application per iteration;
// it delivers the solution up to the east-edge quirk, which phase 2 (BiCGStab on the exact operator, started from here)
// removes in a few iterations.
int SolveRun::pcg_phase()
{
    hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, as, x, r, rhat, p, v, sc);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
    // where PCG hands over: the exact operator's residual of the symmetric problem's solution (the quirk's defect) is
    // ~1e-6 of the right-hand side, so BiCGStab starts from there whatever PCG reached below it
    double reached = 1e300;
    if (pcg(rel_tol, max_iterations, reached) != SSRS_OK)
        return set_error(SSRS_ERR_HIP, "ssrs_potential_solve: HIP error in the PCG phase");
    pcg_ok = reached <= rel_tol;
    SSRS_HIP_CHECK(hipMemcpyAsync(x_pcg, x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (sw.progress) {
        const int rc = report_pcg();
        if (rc != SSRS_OK) return rc;
    }
    // hand over to BiCGStab on the exact operator
    hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, a, x, r, rhat, p, v, sc);
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
    SSRS_HIP_CHECK(hipGetLastError());
    return SSRS_OK;
}

// SSRS_PROGRESS: what PCG's carried residual is worth -- recomputed with the symmetric and with the exact operator
int SolveRun::report_pcg()
{
    for (int q = 0; q < 2; ++q) {
        StencilArgs aq = a;
        aq.quirk = q;
        hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, aq, x, r, rhat, p, v, sc);
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
        SSRS_HIP_CHECK(hipMemcpyAsync(host, &sc->rnorm2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        SSRS_HIP_CHECK(hipStreamSynchronize(st));
        fprintf(stderr, "[ssrs_potential_solve] after PCG (%d iterations): recomputed |r|/|b| %.3e with the %s operator\n", cg_iterations,
                host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : 0.0, q ? "exact (east-edge quirk)" : "symmetric");
        double *dbg = nullptr;
        if (hipMalloc(&dbg, 8 * sizeof(double)) == hipSuccess) {
            (void)hipMemsetAsync(dbg, 0, 8 * sizeof(double), st);
            hipLaunchKernelGGL(k_resid_breakdown, dim3(1024), dim3(kBlock), 0, st, aq, r, dbg);
            double hb[8];
            (void)hipMemcpyAsync(hb, dbg, sizeof(hb), hipMemcpyDeviceToHost, st);
            (void)hipStreamSynchronize(st);
            unsigned long long wcell;
            memcpy(&wcell, &hb[4], sizeof(wcell));
            fprintf(stderr, "    sum r^2: live cells %.3e, dead cells %.3e, east-edge column %.3e (|b|^2 %.3e); largest |r| %.3e at row %llu col %llu\n",
                    hb[0], hb[1], hb[2], host[1], hb[3], wcell / a.cols, wcell % a.cols);
            (void)hipFree(dbg);
        }
    }
    return SSRS_OK;
}

// ---- phase 2 (or the whole solve without the AMG): BiCGStab on the exact operator; x ends as the best iterate
int SolveRun::bicgstab()
{
    int restarts = 0;
    const int check_every = use_amg ? 5 : 25, max_restarts = 50;
    bool fresh = true;                     // p == r (no k_update_p on the first pass)
    // after the PCG phase BiCGStab only has to remove the quirk's defect: it gets what is left of the iteration
    // budget.  (It used to get at least 50 whatever the caller's cap: max_iterations = 5 ran 15 iterations and
    // reported convergence, tests/test_gpu_potential_shapes.py; PCG checks every 5 iterations, so a cap is honoured
    // to the next multiple of 5.)
    int bicg_cap = max_iterations;
    if (use_amg) bicg_cap = max_iterations - cg_iterations > 0 ? max_iterations - cg_iterations : 0;
    // BiCGStab can stagnate under the V(1,1) cycle (snapshot 25 of configs[4]: the carried residual sat at 1.7e-11 for
    // 1 700 iterations, profiles/r04_k5.md) where the V(2,2) cycle of rounds 1-3 converges: a healthy run gains a factor
    // of ten every ~15 iterations, so 40 iterations without a factor of two switch the preconditioner to the
    // robust cycle for the rest of the solve (no restart: x and r stay consistent, only the search directions change)
    bool robust_cycle = false;
    double gain_mark = 1e300;
    int gain_it = 0;
    while (it < bicg_cap) {
        for (int j = 0; j < check_every && it < bicg_cap; ++j, ++it) {
            if (!fresh) hipLaunchKernelGGL(k_update_p, dim3(nb), dim3(kBlock), 0, st, p, r, v, n, sc);
            fresh = false;
            const double *ph = p, *sh = sv;
            if (use_amg) { amg_apply(amg, p, phat, st, robust_cycle); ph = phat; }
            if (a.rinv) hipLaunchKernelGGL(k_apply_dot1_wave, dim3(nb), dim3(kBlock), 0, st, a, ph, v, rhat, sc);
            else hipLaunchKernelGGL(k_apply_dot1, dim3(nb), dim3(kBlock), 0, st, a, ph, v, rhat, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_ALPHA, nb);
            hipLaunchKernelGGL(k_form_s, dim3(nb), dim3(kBlock), 0, st, r, v, sv, n, sc);
            if (use_amg) { amg_apply(amg, sv, shat, st, robust_cycle); sh = shat; }
            if (a.rinv) hipLaunchKernelGGL(k_apply_dot2_wave, dim3(nb), dim3(kBlock), 0, st, a, sh, t, sv, sc);
            else hipLaunchKernelGGL(k_apply_dot2, dim3(nb), dim3(kBlock), 0, st, a, sh, t, sv, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_OMEGA, nb);
            hipLaunchKernelGGL(k_update_xr, dim3(nb), dim3(kBlock), 0, st, x, r, ph, sh, sv, t, rhat, n, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_RHO, nb);
        }
        SSRS_HIP_CHECK(hipGetLastError());
        SSRS_HIP_CHECK(hipMemcpyAsync(host, &sc->rnorm2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        SSRS_HIP_CHECK(hipStreamSynchronize(st));
        const bool finite = host[0] == host[0] && host[0] < 1e300;
        const double now = finite && host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : (finite ? 0.0 : 1e300);
        if (sw.progress && (it % 250 == 0 || sw.progress_every))
            fprintf(stderr, "[ssrs_potential_solve] BiCGStab it %d |r|/|b| %.3e\n", it, now);
        if (finite && now < best) {
            best = now;
            rel = now;
            SSRS_HIP_CHECK(hipMemcpyAsync(xbest, x, n * sizeof(double), hipMemcpyDeviceToDevice, st));
            if (rel <= rel_tol) { converged = 1; break; }
        }
        if (finite && now < 0.5 * gain_mark) { gain_mark = now; gain_it = it; }
        else if (use_amg && !robust_cycle && it - gain_it >= 40) {
            robust_cycle = true;
            robust_from = it;
            gain_it = it;
            if (sw.progress) fprintf(stderr, "[ssrs_potential_solve] BiCGStab it %d: no factor of two in 40 iterations (|r|/|b| %.3e): V(2,2) from here on\n", it, now);
        } else if (use_amg && robust_cycle && pcg_ok && it - gain_it >= 60 && sw.fallback) {
            // stagnation under the robust cycle too (snapshot 25 of configs[4] with the sliced-ELL sweeps' rounding: the
            // residual sat at 5.9e-11 from iteration 200 to the cap at 1 695): no point in waiting for the cap -- the
            // fall-back below takes ~400 PCG iterations from where PCG stood
            if (sw.progress) fprintf(stderr, "[ssrs_potential_solve] BiCGStab it %d: no factor of two in 60 iterations under V(2,2) either (|r|/|b| %.3e)\n", it, now);
            break;
        }
        // BiCGStab breakdown (rho or omega -> 0) or a residual that ran away:
        // restart from the best iterate with a fresh shadow residual
        if (!finite || now > 1e3 * best) {
            if (++restarts > max_restarts) break;
            SSRS_HIP_CHECK(hipMemcpyAsync(x, xbest, n * sizeof(double), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, a, x, r, rhat, p, v, sc);
            hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
            fresh = true;
        }
    }
    if (best < 1e300) SSRS_HIP_CHECK(hipMemcpyAsync(x, xbest, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    return SSRS_OK;
}

// ---- fall-back of phase 2: BiCGStab did not get there (breakdowns, stagnation).  Back to PCG's iterate -- its symmetric
// residual is below rel_tol |b|: taken as zero -- and through the quirk's defect correction (k_quirk_defect) with the
// same PCG: slower than a healthy BiCGStab, but monotone.
int SolveRun::fall_back()
{
    if (sw.progress) fprintf(stderr, "[ssrs_potential_solve] BiCGStab stopped at |r|/|b| %.3e after %d iterations: defect correction from PCG's iterate\n", rel, it);
    SSRS_HIP_CHECK(hipMemcpyAsync(x, x_pcg, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    SSRS_HIP_CHECK(hipMemsetAsync(r, 0, n * sizeof(double), st));
    double *e_prev = rhat;
    SSRS_HIP_CHECK(hipMemsetAsync(e_prev, 0, sizeof(double) * static_cast<size_t>(rows), st));
    const int budget = cg_iterations + max_iterations;           // the fall-back gets an iteration budget of its own
    double dc_last = 1e300;
    for (int dc_rounds = 0; dc_rounds < 40; ++dc_rounds) {
        hipLaunchKernelGGL(k_quirk_defect, dim3((rows + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a, x, e_prev, r);
        hipLaunchKernelGGL(k_norm2, dim3(nb), dim3(kBlock), 0, st, r, n, sc);
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_CG_RR, nb);
        SSRS_HIP_CHECK(hipGetLastError());
        SSRS_HIP_CHECK(hipMemcpyAsync(host, &sc->rnorm2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        SSRS_HIP_CHECK(hipStreamSynchronize(st));
        const double now = host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : 0.0;
        if (sw.progress) fprintf(stderr, "[ssrs_potential_solve] quirk update %d after %d PCG iterations: |r|/|b| %.3e (exact operator)\n", dc_rounds, cg_iterations, now);
        dc_last = now;
        if (now <= rel_tol) { converged = 1; rel = now; break; }
        restart_dirs = true;
        // an update only gains the contraction factor of A_s^-1 E (~0.1): a round solves to a tenth of where it stands
        const double target = now * 0.05 > rel_tol ? now * 0.05 : rel_tol;
        double reached = 1e300;
        if (pcg(target, budget, reached) != SSRS_OK)
            return set_error(SSRS_ERR_HIP, "ssrs_potential_solve: HIP error in the fall-back");
        if (!(reached <= target) || cg_iterations >= budget) break;
    }
    if (!converged) {                      // keep the better of the two unfinished answers
        if (dc_last < rel) rel = dc_last;
        else if (best < 1e300) SSRS_HIP_CHECK(hipMemcpyAsync(x, xbest, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return SSRS_OK;
}

// The f32 potential and the stats
int SolveRun::finish(void *stats_out)
{
    if (sw.progress) {
        // the residual the iteration carried along against the one recomputed from x
        hipLaunchKernelGGL(k_setup, dim3(nb), dim3(kBlock), 0, st, a, x, r, rhat, p, v, sc);
        hipLaunchKernelGGL(k_finish, dim3(1), dim3(kBlock), 0, st, sc, FIN_INIT, nb);
        SSRS_HIP_CHECK(hipMemcpyAsync(host, &sc->rnorm2, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        SSRS_HIP_CHECK(hipStreamSynchronize(st));
        fprintf(stderr, "[ssrs_potential_solve] done: carried |r|/|b| %.3e, recomputed %.3e (PCG %d + BiCGStab %d iterations%s)\n", rel,
                host[1] > 0.0 ? std::sqrt(host[0] / host[1]) : 0.0, cg_iterations, it, robust_from >= 0 ? ", the last of them under V(2,2)" : "");
    }
    if (converged) {
        hipLaunchKernelGGL(k_to_f32, dim3(nb), dim3(kBlock), 0, st, x, potential, n);
    } else {                               // (the reduction partials are free by now)
        hipLaunchKernelGGL(k_dirichlet_range, dim3(1), dim3(kBlock), 0, st, fixed, fixed_values, n, &sc->part[0][0]);
        hipLaunchKernelGGL(k_to_f32_clamped, dim3(nb), dim3(kBlock), 0, st, x, potential, n, &sc->part[0][0]);
    }
    SSRS_HIP_CHECK(hipGetLastError());
    SSRS_HIP_CHECK(hipEventRecord(ev.last, st));
    SSRS_HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.first, ev.last);
    if (stats_out) {
        auto *so = static_cast<SsrsSolveStatsInternal *>(stats_out);
        so->iterations = it + cg_iterations;
        so->converged = converged;
        so->residual = rel;
        so->kernel_ms = ms;
        so->amg_levels = use_amg ? static_cast<int32_t>(amg.levels.size()) : 0;
        so->amg_coarsest = use_amg ? amg.levels.back().n : 0;
        so->setup_ms = setup_ms;
        so->workspace_used = ws_used;
    }
    return SSRS_OK;
}

}  // namespace

extern "C" int ssrs_potential_solve(const double *conductivity, const uint8_t *fixed_mask,
                                    const double *fixed_values, const double *initial_guess,
                                    float *potential, int rows, int cols, double rel_tol,
                                    int max_iterations, int flags, void *workspace,
                                    size_t workspace_bytes, void *stats_out, void *stream)
{
    SSRS_REQUIRE(conductivity && fixed_mask && fixed_values && potential && workspace,
                 "ssrs_potential_solve: NULL pointer");
    SSRS_REQUIRE(rows >= 3 && cols >= 3, "ssrs_potential_solve: need rows, cols >= 3");
    // ssrs_potential_workspace_bytes is the bound that always suffices; a smaller workspace is
    // accepted as long as the solver's own vectors fit, and the hierarchy reports "workspace
    // exhausted" if it does not (it really takes ~840 B per cell)
    SSRS_REQUIRE(workspace_bytes >= (sizeof(Scalars) + 255) / 256 * 256 + 11 * vec_bytes(static_cast<size_t>(rows) * cols) + 512,
                 "ssrs_potential_solve: workspace too small");
    SSRS_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255u) == 0,
                 "ssrs_potential_solve: workspace must be 256-byte aligned");
    SSRS_REQUIRE(rel_tol > 0.0 && max_iterations > 0, "ssrs_potential_solve: bad tolerance / iteration cap");
    // The solve is synchronous (it returns after its last kernel), so when the caller
    // hands over the null stream the work runs on a private stream instead: graph
    // capture of the V-cycle needs a capturable stream.  Caller order is kept by an
    // event wait at entry and a stream sync at exit.
    hipStream_t st = as_stream(stream);
    if (st == nullptr) {
        static thread_local hipStream_t own = nullptr;
        if (!own && hipStreamCreateWithFlags(&own, hipStreamNonBlocking) != hipSuccess) own = nullptr;
        if (own) {
            SSRS_HIP_CHECK(hipStreamSynchronize(nullptr));   // everything queued before the call
            st = own;
        }
    }
    SolveRun run(conductivity, fixed_mask, fixed_values, initial_guess, potential, rows, cols, rel_tol, max_iterations, flags,
                 workspace, workspace_bytes, st);
    int rc;
    if (run.use_amg && (rc = run.setup_amg()) != SSRS_OK) return rc;
    if ((rc = run.start()) != SSRS_OK) return rc;
    if (run.use_amg && (rc = run.pcg_phase()) != SSRS_OK) return rc;
    if ((rc = run.bicgstab()) != SSRS_OK) return rc;
    if (run.use_amg && !run.converged && run.pcg_ok && run.sw.fallback && (rc = run.fall_back()) != SSRS_OK) return rc;
    return run.finish(stats_out);
}
