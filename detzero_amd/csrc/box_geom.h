// Rotated-rectangle geometry shared by the kernels that need BEV overlaps (head_post.hip: IoU matrices, NMS;
// wbf.hip: box fusion; box_ops.hip: 3-D IoU / GIoU matrices, which also need the convex hull of two footprints).
// Formula sequence of utils/detzero_utils/ops/iou3d_nms/src/iou3d_nms_kernel.cu:15-232,328-335 in fp32; include it
// AFTER `#pragma clang fp contract(off)` so that discrete decisions (IoU > thr) agree with the CPU restatement
// wherever libm and ocml agree on sin/cos/atan2.
#pragma once
#include "common.h"

namespace dz {

// ------------------------------------------------------------------------------------------
// rotated rectangle overlap
// ------------------------------------------------------------------------------------------
struct P2 { float x, y; };
constexpr float GEO_EPS = 1e-8f;

__device__ __forceinline__ float cr2(P2 a, P2 b) { return a.x * b.y - a.y * b.x; }
__device__ __forceinline__ float cr3(P2 p1, P2 p2, P2 p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}
__device__ __forceinline__ bool bbox_cross(P2 p1, P2 p2, P2 q1, P2 q2) {
    return fminf(p1.x, p2.x) <= fmaxf(q1.x, q2.x) && fminf(q1.x, q2.x) <= fmaxf(p1.x, p2.x) &&
           fminf(p1.y, p2.y) <= fmaxf(q1.y, q2.y) && fminf(q1.y, q2.y) <= fmaxf(p1.y, p2.y);
}
__device__ __forceinline__ bool corner_in_box(const float *box, P2 p) {
    const float MARGIN = 1e-2f;
    const float cx = box[0], cy = box[1];
    const float ac = cosf(-box[6]), as = sinf(-box[6]);
    const float rx = (p.x - cx) * ac + (p.y - cy) * (-as);
    const float ry = (p.x - cx) * as + (p.y - cy) * ac;
    return fabsf(rx) < box[3] / 2 + MARGIN && fabsf(ry) < box[4] / 2 + MARGIN;
}
__device__ __forceinline__ bool edge_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2 &ans) {
    if (!bbox_cross(p0, p1, q0, q1)) return false;
    const float s1 = cr3(q0, p1, p0);
    const float s2 = cr3(p1, q1, p0);
    const float s3 = cr3(p0, q1, q0);
    const float s4 = cr3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cr3(q1, p1, p0);
    if (fabsf(s5 - s1) > GEO_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}
__device__ __forceinline__ void spin(P2 c, float ac, float as, P2 &p) {
    const float nx = (p.x - c.x) * ac + (p.y - c.y) * (-as) + c.x;
    const float ny = (p.x - c.x) * as + (p.y - c.y) * ac + c.y;
    p.x = nx; p.y = ny;
}

// Intersection polygon vertices live in LDS (column `tid` of a [16][nthreads] array): a dynamically
// indexed private array would be spilled to scratch memory, which we avoid in every kernel so that
// whole frames replay from hipGraphs without a scratch segment.
__device__ float rect_overlap(const float *A, const float *B, P2 *cp, float *ang, int ld) {
    const float adx = A[3] / 2, bdx = B[3] / 2, ady = A[4] / 2, bdy = B[4] / 2;
    const P2 ca{A[0], A[1]}, cb{B[0], B[1]};
    P2 a0{A[0] - adx, A[1] - ady}, a1{A[0] + adx, A[1] - ady}, a2{A[0] + adx, A[1] + ady}, a3{A[0] - adx, A[1] + ady};
    P2 b0{B[0] - bdx, B[1] - bdy}, b1{B[0] + bdx, B[1] - bdy}, b2{B[0] + bdx, B[1] + bdy}, b3{B[0] - bdx, B[1] + bdy};
    const float acs = cosf(A[6]), asn = sinf(A[6]), bcs = cosf(B[6]), bsn = sinf(B[6]);
    spin(ca, acs, asn, a0); spin(ca, acs, asn, a1); spin(ca, acs, asn, a2); spin(ca, acs, asn, a3);
    spin(cb, bcs, bsn, b0); spin(cb, bcs, bsn, b1); spin(cb, bcs, bsn, b2); spin(cb, bcs, bsn, b3);
    const P2 ac[5] = {a0, a1, a2, a3, a0};     // constant indices only after full unrolling -> registers
    const P2 bc[5] = {b0, b1, b2, b3, b0};

    P2 pc{0.f, 0.f};
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            P2 t;
            if (edge_cross(ac[i + 1], ac[i], bc[j + 1], bc[j], t)) {
                cp[cnt * ld] = t; pc.x = pc.x + t.x; pc.y = pc.y + t.y; ++cnt;
            }
        }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (corner_in_box(A, bc[k])) { pc.x = pc.x + bc[k].x; pc.y = pc.y + bc[k].y; cp[cnt * ld] = bc[k]; ++cnt; }
        if (corner_in_box(B, ac[k])) { pc.x = pc.x + ac[k].x; pc.y = pc.y + ac[k].y; cp[cnt * ld] = ac[k]; ++cnt; }
    }
    pc.x /= cnt; pc.y /= cnt;   // cnt == 0 gives NaN exactly as the reference; the loops below do not run
    // bubble sort by polar angle around the centroid (angles cached; comparisons identical)
    for (int i = 0; i < cnt; ++i) ang[i * ld] = atan2f(cp[i * ld].y - pc.y, cp[i * ld].x - pc.x);
    for (int j = 0; j < cnt - 1; ++j)
        for (int i = 0; i < cnt - j - 1; ++i) {
            const float x0 = ang[i * ld], x1 = ang[(i + 1) * ld];
            if (x0 > x1) {
                const P2 t = cp[i * ld]; cp[i * ld] = cp[(i + 1) * ld]; cp[(i + 1) * ld] = t;
                ang[i * ld] = x1; ang[(i + 1) * ld] = x0;
            }
        }
    float area = 0.f;
    const P2 c0 = cp[0];
    for (int k = 0; k < cnt - 1; ++k) {
        const P2 ck = cp[k * ld], cn = cp[(k + 1) * ld];
        const P2 u{ck.x - c0.x, ck.y - c0.y};
        const P2 v{cn.x - c0.x, cn.y - c0.y};
        area += cr2(u, v);
    }
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float rect_iou(const float *A, const float *B, P2 *cp, float *ang, int ld) {
    const float sa = A[3] * A[4], sb = B[3] * B[4];
    const float so = rect_overlap(A, B, cp, ang, ld);
    return so / fmaxf(sa + sb - so, GEO_EPS);
}

// ------------------------------------------------------------------------------------------
// convex hull of two rotated rectangles
// ------------------------------------------------------------------------------------------
// compare-exchange into lexicographic (x, then y) order
__device__ __forceinline__ void lex_cswap(P2 &a, P2 &b) {
    const bool sw = b.x < a.x || (b.x == a.x && b.y < a.y);
    const P2 t = a;
    if (sw) { a = b; b = t; }
}

// Area of the convex hull of the eight corners of A and B: what boxes_union_kernel / box_union
// (iou3d_nms_kernel.cu:235-326,352-368) is meant to compute.  That walk reads hull[0] without ever writing it
// (:288-316), so it is NOT transcribed: this is the mathematical hull area in fp32.  Corners exactly as rect_overlap
// builds them; the sort is a 19-exchange network on registers (constant indices only); monotone chain that pops on
// cross <= 0, so collinear and duplicate corners drop out; shoelace relative to the first hull vertex.  The hull
// stack is column `tid` of a [9][nthreads] LDS array (`stk`, stride `ld`), by the rule stated above rect_overlap.
__device__ float rect_hull_area(const float *A, const float *B, P2 *stk, int ld) {
    const float adx = A[3] / 2, bdx = B[3] / 2, ady = A[4] / 2, bdy = B[4] / 2;
    const P2 ca{A[0], A[1]}, cb{B[0], B[1]};
    P2 a0{A[0] - adx, A[1] - ady}, a1{A[0] + adx, A[1] - ady}, a2{A[0] + adx, A[1] + ady}, a3{A[0] - adx, A[1] + ady};
    P2 b0{B[0] - bdx, B[1] - bdy}, b1{B[0] + bdx, B[1] - bdy}, b2{B[0] + bdx, B[1] + bdy}, b3{B[0] - bdx, B[1] + bdy};
    const float acs = cosf(A[6]), asn = sinf(A[6]), bcs = cosf(B[6]), bsn = sinf(B[6]);
    spin(ca, acs, asn, a0); spin(ca, acs, asn, a1); spin(ca, acs, asn, a2); spin(ca, acs, asn, a3);
    spin(cb, bcs, bsn, b0); spin(cb, bcs, bsn, b1); spin(cb, bcs, bsn, b2); spin(cb, bcs, bsn, b3);
    P2 p[8] = {a0, a1, a2, a3, b0, b1, b2, b3};     // constant indices only after full unrolling -> registers
    lex_cswap(p[0], p[2]); lex_cswap(p[1], p[3]); lex_cswap(p[4], p[6]); lex_cswap(p[5], p[7]);
    lex_cswap(p[0], p[4]); lex_cswap(p[1], p[5]); lex_cswap(p[2], p[6]); lex_cswap(p[3], p[7]);
    lex_cswap(p[0], p[1]); lex_cswap(p[2], p[3]); lex_cswap(p[4], p[5]); lex_cswap(p[6], p[7]);
    lex_cswap(p[2], p[4]); lex_cswap(p[3], p[5]);
    lex_cswap(p[1], p[4]); lex_cswap(p[3], p[6]);
    lex_cswap(p[1], p[2]); lex_cswap(p[3], p[4]); lex_cswap(p[5], p[6]);

    int k = 0;      // lower chain, left to right: at most 8 entries
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        while (k >= 2 && cr3(stk[(k - 1) * ld], p[i], stk[(k - 2) * ld]) <= 0.f) --k;
        stk[k * ld] = p[i]; ++k;
    }
    const int floor_k = k + 1;      // upper chain, right to left, on top of the lower one; it ends on p[0] again
#pragma unroll
    for (int i = 6; i >= 0; --i) {
        while (k >= floor_k && cr3(stk[(k - 1) * ld], p[i], stk[(k - 2) * ld]) <= 0.f) --k;
        if (k < 9) { stk[k * ld] = p[i]; ++k; }     // a hull of 8 points has <= 8 vertices + the repeated first; NaN corners never pop
    }
    float area = 0.f;
    const P2 h0 = stk[0];
    for (int j = 1; j < k - 2; ++j) {
        const P2 hj = stk[j * ld], hn = stk[(j + 1) * ld];
        const P2 u{hj.x - h0.x, hj.y - h0.y};
        const P2 v{hn.x - h0.x, hn.y - h0.y};
        area += cr2(u, v);
    }
    return fabsf(area) / 2.0f;
}

// ------------------------------------------------------------------------------------------
// pair metrics
// ------------------------------------------------------------------------------------------
// true when the circumscribed circles of the two footprints are at most 5 cm apart (k_nms_mask's test): beyond that
// rect_overlap finds no vertex (its corner test has a 1 cm margin) and returns exactly +0
__device__ __forceinline__ bool footprints_near(const float *A, const float *B) {
    const float dx = A[0] - B[0], dy = A[1] - B[1];
    const float reach = sqrtf(0.25f * (A[3] * A[3] + A[4] * A[4])) + sqrtf(0.25f * (B[3] * B[3] + B[4] * B[4])) + 0.05f;
    return dx * dx + dy * dy <= reach * reach;
}

// One pair, the final value of a DZ_BOXM_* metric: the one body of box_ops.hip's matrix and paired kernels and of track.hip's
// affinity kernel, so that their results agree bit for bit.  cp / ang = the thread's LDS columns (stride ld).
template <int METRIC>
__device__ __forceinline__ float pair_metric_ld(const float *A, const float *B, P2 *cp, float *ang, int ld) {
    if (METRIC == DZ_BOXM_UNION_BEV) return rect_hull_area(A, B, cp, ld);
    // iou3d_nms_utils.py:86-105 / :122-150, operation for operation
    const float a_max = A[2] + A[5] / 2, a_min = A[2] - A[5] / 2;
    const float b_max = B[2] + B[5] / 2, b_min = B[2] - B[5] / 2;
    const float bev = footprints_near(A, B) ? rect_overlap(A, B, cp, ang, ld) : 0.f;
    const float oh = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
    const float o3 = bev * oh;
    const float va = (A[3] * A[4]) * A[5], vb = (B[3] * B[4]) * B[5];
    const float u3 = fmaxf((va + vb) - o3, 1e-6f);
    if (METRIC == DZ_BOXM_IOU3D) return o3 / u3;
    // the reference's enclosing height is min(tops) - min(bottoms) (:139 `max_of_max = torch.min(...)`); EXACT = max(tops) - min(bottoms)
    const float top = METRIC == DZ_BOXM_GIOU3D_EXACT ? fmaxf(a_max, b_max) : fminf(a_max, b_max);
    const float uh = fmaxf(top - fminf(a_min, b_min), 0.f);
    const float c3 = fmaxf(rect_hull_area(A, B, cp, ld) * uh, 1e-6f);
    return o3 / u3 - (c3 - u3) / c3;
}

}  // namespace dz
