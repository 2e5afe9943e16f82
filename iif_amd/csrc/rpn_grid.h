// The anchor grid and the sampled index lists of the RPN head's training side, shared by rpn_stage.hip (targets, loss) and
// rpn_head_sampled.hip (the head's backward at the sampled pixels): the by-value level table, flat index -> (level, y, x, a),
// and slot e of the B (nep + num) entries -> flat anchor index.
#pragma once
#include "common.h"

namespace {

constexpr int kMaxImages = 16;
constexpr int kMaxLevels = 8;
constexpr int kMaxBase = 16;
constexpr int kMaxNum = 1024;

struct Lvl { int start, W, H, nb, sx, sy; };
struct Grid { int L, A; Lvl lv[kMaxLevels]; };
struct Bases { float b[kMaxLevels][kMaxBase][4]; };

struct Cell { int l, x, y, a, r; };

__device__ __forceinline__ Cell locate(const Grid& g, int i) {
    Cell c;
    c.l = 0;
    for (int k = 1; k < g.L; ++k)
        if (i >= g.lv[k].start) c.l = k;
    const Lvl& v = g.lv[c.l];
    c.r = i - v.start;
    c.a = c.r % v.nb;
    const int cell = c.r / v.nb;
    c.x = cell % v.W;
    c.y = cell / v.W;
    return c;
}

bool fill_grid(const iif_rpn_grid* in, Grid* g, Bases* bs) {
    if (!in || in->num_levels < 1 || in->num_levels > kMaxLevels) return false;
    int64_t at = 0;
    g->L = in->num_levels;
    for (int l = 0; l < in->num_levels; ++l) {
        const int W = in->W[l], H = in->H[l], nb = in->num_base[l];
        if (W < 0 || H < 0 || W > 65535 || H > 65535 || nb < 1 || nb > kMaxBase || in->stride_w[l] < 1 || in->stride_h[l] < 1) return false;
        if ((int64_t)W * in->stride_w[l] >= (1 << 24) || (int64_t)H * in->stride_h[l] >= (1 << 24)) return false;   // exact as float32
        g->lv[l] = Lvl{(int)at, W > 0 ? W : 1, H, nb, in->stride_w[l], in->stride_h[l]};
        at += (int64_t)W * H * nb;
        if (at >= INT32_MAX - 4) return false;
        if (bs)
            for (int a = 0; a < nb; ++a)
                for (int j = 0; j < 4; ++j) bs->b[l][a][j] = in->base[l][a][j];
    }
    g->A = (int)at;
    return true;
}

// ------------------------------------------------------------------------------------------------ the sampled lists
struct Lists { const int64_t* pos_inds; const int64_t* neg_inds; const int64_t* counts; const float* pos_bt; int nep, num, B; };

__device__ __forceinline__ int clampi(int64_t v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// entry e of the B (nep + num) slots: the flat anchor index, or -1 for an unused slot
__device__ __forceinline__ int64_t entry_of(const Lists& s, int e, int& b, bool& pos, int& slot) {
    const int per = s.nep + s.num;
    b = e / per;
    const int r = e - b * per;
    pos = r < s.nep;
    slot = pos ? r : r - s.nep;
    const int kp = clampi(s.counts[2 * b], s.nep), kn = clampi(s.counts[2 * b + 1], s.num);
    if (slot >= (pos ? kp : kn)) return -1;
    return pos ? s.pos_inds[(int64_t)b * s.nep + slot] : s.neg_inds[(int64_t)b * s.num + slot];
}

bool fill_lists(Lists* s, int B, const int64_t* pos_inds, const int64_t* neg_inds, const int64_t* counts, const float* pos_bt,
                int64_t nep, int64_t num) {
    if (B < 1 || B > kMaxImages || num < 0 || num > kMaxNum || nep < 0 || nep > num || !counts) return false;
    if ((nep > 0 && (!pos_inds || !pos_bt)) || (num > 0 && !neg_inds)) return false;
    if (!aligned_to(pos_inds, 8) || !aligned_to(neg_inds, 8) || !aligned_to(counts, 8) || !aligned_to(pos_bt, 16)) return false;
    s->pos_inds = pos_inds; s->neg_inds = neg_inds; s->counts = counts; s->pos_bt = pos_bt;
    s->nep = (int)nep; s->num = (int)num; s->B = B;
    return true;
}

}  // namespace
