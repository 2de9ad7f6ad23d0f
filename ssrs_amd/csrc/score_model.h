// The movement model as the track scores restate it (K21 score.hip, K22 score_profile.hip): the restriction masks, the
// burn-in relocation, numpy's pairwise sum of nine, the raw 3 x 3 window weights and the probability sequence, RESTATED from
// tracks.hip (window_weights, restriction, choose_move's exact branch), not shared with it.  Both kernels include this file,
// so that one move gets one arithmetic: -ffp-contract=off is required, every division is a division, sum9 keeps numpy's
// pairwise order.  score_window_weights reads updraft, potential, cols and prior[9] of the kernel's own argument block.
#pragma once
#include <cstdint>

#include "common.h"
#include "../../include/ssrs_score.h"

namespace ssrs {

typedef unsigned long long u64;
// the stage of a tile of kBlock points in LDS, and the counts of a block packed beside its surprisal
constexpr int kScoreBack = 8;                              // points staged behind the tile: the deepest look-back
constexpr int kScoreAhead = 4;                             // points staged ahead of it: the next point of the last lane
constexpr int kScoreStage = kScoreBack + kBlock + kScoreAhead;
constexpr int kScoreCountBits = 12;                        // a block holds at most kBlock = 256 moves of one status
constexpr uint32_t kScoreAllButCentre = 0x1EFu;
static_assert(kScoreBack % 4 == 0 && kScoreAhead % 4 == 0 && kBlock % 4 == 0, "the stage is whole 16-byte loads");
static_assert(kScoreBack >= SSRS_SCORE_MAX_MEMORY, "the look-back stays inside the stage");
static_assert(kBlock < (1 << kScoreCountBits) && 5 * kScoreCountBits <= 64, "the packed counts cannot carry");

// movmodel.py:185-202: the cells within +-45 degrees of the move (dr, dc); (0, 0) allows all; never the centre
__host__ __device__ __forceinline__ uint32_t score_restriction(int dr, int dc)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int kr = k / 3 - 1, kc = k % 3 - 1;
        bool ok;
        if (dr == 0 && dc == 0) ok = true;
        else if (dr != 0 && dc != 0) ok = (kr == dr || kr == 0) && (kc == dc || kc == 0);
        else if (dr == 0) ok = kc == dc;
        else ok = kr == dr;
        if (ok && k != 4) m |= 1u << k;
    }
    return m;
}

// movmodel.py:205-217 (asymmetric on purpose: row <= 1 but col <= 0)
__host__ __device__ __forceinline__ void score_move_away(int rows, int cols, int &r, int &c)
{
    if (r <= 1) r += 2;
    else if (r >= rows - 2) r -= 2;
    if (c <= 0) c += 2;
    else if (c >= cols - 2) c -= 2;
}

__host__ __device__ __forceinline__ double score_sum9(const double *x)
{   // numpy pairwise summation for n = 9
    return (((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))) + x[8];
}

// the raw 3 x 3 move weights of movmodel.py:292-306 at the interior cell (row, col)
template <class Args>
__device__ __forceinline__ void score_window_weights(const Args &a, int row, int col, double *w)
{
    if (a.updraft == nullptr) {
#pragma unroll
        for (int j = 0; j < 9; ++j) w[j] = a.prior[j];
        return;
    }
    const long long centre = static_cast<long long>(row) * a.cols + col;
    double win[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        const double v = a.updraft[centre + (j / 3 - 1) * a.cols + (j % 3 - 1)];
        win[j] = v != v ? v : (v > 1e-06 ? v : 1e-06);             // clip(min=1e-06), NaN kept
    }
    const double ic = 1.0 / win[4];
#pragma unroll
    for (int j = 0; j < 9; ++j) w[j] = 2.0 / (ic + 1.0 / win[j]);   // harmonic mean with the centre
    if (a.potential != nullptr) {
        const float pc = a.potential[centre];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float d = pc - a.potential[centre + (j / 3 - 1) * a.cols + (j % 3 - 1)];
            const float ninv = (j == 4) ? 0.f : ((j & 1) ? 1.f : 0.70710677f);     // f32(1 / sqrt(2)) as the reference stores it
            const float e = d * ninv;                              // stays f32
            w[j] = w[j] * static_cast<double>(e);
        }
    }
}

// generate_move_probabilities (movmodel.py:220-244), the half that does not depend on nu: q[9] from the raw weights w[9]
// through the NaN rule, the clip, the mask, both prior fall-backs and the first normalisation
__device__ __forceinline__ void score_probabilities_head(const double *w, const double *prior, uint32_t mask, double *q)
{
    bool has_nan = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) has_nan |= (w[k] != w[k]);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double v = has_nan ? prior[k] : w[k];
        q[k] = v > 0.0 ? v : 0.0;                                  // clip(min=0)
    }
    q[4] = 0.0;
    bool any = false;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double z = q[k] * 0.0;                               // ix * float(iy): inf becomes NaN
        q[k] = ((mask >> k) & 1u) ? q[k] : z;
        any |= (q[k] != 0.0);
    }
    if (!any) {                                                    // all masked weights are zero: the masked prior
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            q[k] = ((mask >> k) & 1u) && k != 4 ? prior[k] : 0.0;
            any |= (q[k] != 0.0);
        }
        if (!any) {                                                // the prior fully masked as well
#pragma unroll
            for (int k = 0; k < 9; ++k) q[k] = prior[k];
        }
    }
    const double s1 = score_sum9(q);
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = q[k] / s1;
}

// generate_move_probabilities (movmodel.py:220-244): q[9] from the raw weights w[9]
__device__ __forceinline__ void score_probabilities(const double *w, const double *prior, double nu, uint32_t mask, double *q)
{
    score_probabilities_head(w, prior, mask, q);
    if (nu != 1.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = pow(q[k], nu);
    }
    const double s2 = score_sum9(q);
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = q[k] / s2;
}

// the other half for ONE cell: entry idx of score_probabilities' q[9] from the head's q1[9] -- the nine pow (none when nu
// is 1), the second pairwise sum and the one division q[idx] / s2, the same operations on the same operands
__device__ __forceinline__ double score_probability_of(const double *q1, double nu, int idx)
{
    double q[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) q[k] = q1[k];
    if (nu != 1.0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) q[k] = pow(q[k], nu);
    }
    const double s2 = score_sum9(q);
    double qi = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) qi = k == idx ? q[k] : qi;
    return qi / s2;
}

}  // namespace ssrs
