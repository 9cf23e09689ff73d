// The per-cell arithmetic of the triangle mesh from depth (gp_depth_mesh; definition in include/genpercept_hip.h), written once for the
// device kernels of depth_mesh.hip and for a CPU program (tests/mesh_check.cpp): the link test of two nodes, the diagonal and the four-bit
// code of a cell, which triangles use a node, the corners of a triangle and the texture coordinate of a pixel.  No HIP header is needed.
// Everything is float64, the operations are - fabs min * and compares in the order written, and nothing may be contracted into a fused
// multiply-add (genpercept_amd/mesh.py is numpy).
//
// Definition, per image.  Node (gy, gx) of the stride grid is pixel (v, u) = (gy stride, gx stride); k = keep != 0, z = plane 2 of xyz as float64.
//   link   p and q are linked iff k_p, k_q and |z_p - z_q| <= cut * min(z_p, z_q); a NaN fails the test.
//   cell   (cy, cx), cy < gh - 1, cx < gw - 1: corners a = (cy, cx), b = (cy, cx + 1), c = (cy + 1, cx), d = (cy + 1, cx + 1).
//          T0 = (a, c, d), T1 = (a, d, b) on diagonal a-d; T2 = (a, c, b), T3 = (b, c, d) on diagonal b-c.  The cell uses a-d iff k_a, k_d and
//          (not (k_b and k_c), or |z_a - z_d| <= |z_b - z_c|); otherwise b-c.  It emits the triangles of its diagonal whose three edges are
//          all linked.  code = T0 | T1 << 1 | T2 << 2 | T3 << 3, one of 0, 1, 2, 3, 4, 8, 12.
//   The corner orders make (v1 - v0) x (v2 - v0) point to the camera (x right, y down, z forward, the camera at the origin).
#pragma once

#include <math.h>

#include "depth_geometry_math.h"   // DG_HD, DG_MAX_DIM, DG_MAX_STRIDE

#pragma clang fp contract(off)

constexpr long long DM_MAX_NODES = 1LL << 30;   // B gh gw < 2^30: the triangle count stays below 2^31

// cut in (0, 1]; false for a NaN
DG_HD bool dm_cut_ok(double cut) { return cut > 0.0 && cut <= 1.0; }

DG_HD bool dm_linked(bool kp, double zp, bool kq, double zq, double cut) {
    if (!kp || !kq) return false;
    const double d = fabs(zp - zq);
    const double m = zp < zq ? zp : zq;
    const double lim = cut * m;
    return d <= lim;
}

// the code of the cell with the corners a, b, c, d
DG_HD unsigned dm_cell_code(bool ka, double za, bool kb, double zb, bool kc, double zc, bool kd, double zd, double cut) {
    const bool ab = dm_linked(ka, za, kb, zb, cut), ac = dm_linked(ka, za, kc, zc, cut);
    const bool bd = dm_linked(kb, zb, kd, zd, cut), cd = dm_linked(kc, zc, kd, zd, cut);
    const bool use_ad = ka && kd && (!(kb && kc) || fabs(za - zd) <= fabs(zb - zc));
    if (use_ad) {
        const bool ad = dm_linked(ka, za, kd, zd, cut);
        return (ad && ac && cd ? 1u : 0u) | (ad && bd && ab ? 2u : 0u);
    }
    const bool bc = dm_linked(kb, zb, kc, zc, cut);
    return (bc && ac && ab ? 4u : 0u) | (bc && cd && bd ? 8u : 0u);
}

// the bits of a cell's code whose triangles use its corner a, b, c, d
constexpr unsigned DM_USES_A = 7u, DM_USES_B = 14u, DM_USES_C = 13u, DM_USES_D = 11u;

// A node is a vertex iff a triangle of one of its four cells uses it: code_a is the code of the cell whose corner a it is (the cell at the
// node itself), code_b that of the cell to its left, code_c above, code_d above left; 0 where there is no such cell.
DG_HD bool dm_node_used(unsigned code_a, unsigned code_b, unsigned code_c, unsigned code_d) {
    return ((code_a & DM_USES_A) | (code_b & DM_USES_B) | (code_c & DM_USES_C) | (code_d & DM_USES_D)) != 0u;
}

// how many triangles a code emits
DG_HD int dm_code_count(unsigned code) { return (int)((code & 5u) != 0u) + (int)((code & 10u) != 0u); }

// Triangle `slot` (0: T0 or T2, the first the cell emits of its diagonal's two; 1: T1 or T3) of a cell with the vertex indices a, b, c, d of
// its corners: whether the code holds it, and its corners in order.
DG_HD bool dm_triangle(unsigned code, int slot, int a, int b, int c, int d, int (&t)[3]) {
    if (slot == 0) {
        if (code & 1u) return t[0] = a, t[1] = c, t[2] = d, true;
        if (code & 4u) return t[0] = a, t[1] = c, t[2] = b, true;
        return false;
    }
    if (code & 2u) return t[0] = a, t[1] = d, t[2] = b, true;
    if (code & 8u) return t[0] = b, t[1] = c, t[2] = d, true;
    return false;
}

// the texture coordinate of pixel u of n: (u + 0.5) / n in float64, rounded once to float32
DG_HD float dm_uv(int u, int n) { return (float)(((double)u + 0.5) / (double)n); }
