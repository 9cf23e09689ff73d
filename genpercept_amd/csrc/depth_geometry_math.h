// The per-pixel arithmetic of the depth geometry (gp_depth_geometry; definition in include/genpercept_hip.h), written once for the device
// kernels of depth_geometry.hip and for a CPU program (tests/geometry_check.cpp): the depth of a pixel from its 16-bit value, the membership
// test and the sums of the plane fit in inverse depth, the solve, the point, the normal and the keep decision.  No HIP header is needed.  The
// quantisation is gs_quant16 of guided_solve.h.  Everything after it is float64, the operations are + - * / sqrt in the order written, and
// nothing may be contracted into a fused multiply-add (genpercept_amd/geometry.py is numpy).
//
// Definition, per image.  pred float32 [1][H][W]; mask uint8 [H][W] or none (non-zero: usable); the camera is eight float64 values
// s, t, fx, fy, cx, cy, z_min, z_max (OpenCV's: x right, y down, z forward, pixel (u, v) has its centre at integer (u, v)).
//   1. Q = gs_quant16(pred); lin = s * (Q / 65535) + t; z = lin (depth) or 1 / lin (disparity).  A pixel is valid iff pred is not NaN, the
//      mask is not 0, z is finite and z_min <= z <= z_max.  w = 1 / z.
//   2. X = ((u - cx) / fx) * z, Y = ((v - cy) / fy) * z, Z = z, each rounded once to float32; NaN for an invalid pixel.
//   3. The members of valid pixel i are the valid pixels j of its (2 r + 1)^2 window, clipped to the image, with |z_j - z_i| <= tau * z_i.
//      In row-major order, du = u_j - u_i, dv = v_j - v_i: the integers n, Su, Sv, Suu, Suv, Svv and the float64 sums Sw, Suw, Svw
//      (from +0.0, one product and one add per member).  [[Suu, Suv, Su], [., Svv, Sv], [., ., n]] (a, b, c) = (Suw, Svw, Sw) by cofactors
//      (dg_solve).  The fit is valid iff n >= min_count and det > 0.  m = (a fx, b fy, (c + a (cx - u_i)) + b (cy - v_i)).
//   4. N_k = -m_k / sqrt((m0^2 + m1^2) + m2^2), rounded once to float32; (0, 0, 0) where the fit is invalid or the norm is 0 or not finite.
//   5. kept iff valid, the fit valid, and with p = ((u - cx) / fx, (v - cy) / fy, 1), mp = (m0 p0 + m1 p1) + m2 p2:
//      mp * mp >= ((min_cos * min_cos) * ((m0^2 + m1^2) + m2^2)) * ((p0^2 + p1^2) + 1) and mp > 0.
#pragma once

#include <math.h>

#include "guided_solve.h"

#pragma clang fp contract(off)

#define DG_HD GS_HD

constexpr int DG_MAX_DIM = 16384;   // 1 <= H, W <= 16384
constexpr int DG_MAX_R = 8;         // 1 <= r <= 8: every cofactor and the determinant are exact integers below 2^53
constexpr int DG_MAX_STRIDE = 64;   // 1 <= stride <= 64
constexpr int DG_CAMERA = 8;        // s, t, fx, fy, cx, cy, z_min, z_max
enum { DG_SPACE_DEPTH = 0, DG_SPACE_DISPARITY = 1 };

struct DgCamera {
    double s, t, fx, fy, cx, cy, z_min, z_max;
};

DG_HD bool dg_finite(double x) { return x - x == 0.0; }

// the eight values are finite, fx, fy > 0 and 0 < z_min < z_max
DG_HD bool dg_camera_ok(const double* c) {
    for (int k = 0; k < DG_CAMERA; ++k)
        if (!dg_finite(c[k])) return false;
    return c[2] > 0.0 && c[3] > 0.0 && c[6] > 0.0 && c[6] < c[7];
}

// the ranges of the call
DG_HD bool dg_options_ok(int space, int r, double tau, int min_count, double min_cos, int stride) {
    return (space == DG_SPACE_DEPTH || space == DG_SPACE_DISPARITY) && r >= 1 && r <= DG_MAX_R && tau > 0.0 && tau <= 1.0 && min_count >= 3 &&
           min_count <= (2 * r + 1) * (2 * r + 1) && min_cos >= 0.0 && min_cos < 1.0 && stride >= 1 && stride <= DG_MAX_STRIDE;
}

// Step 1.  Returns the pixel's validity; z and w = 1 / z are meaningful for a valid pixel only.
DG_HD bool dg_depth(float pred, bool usable, const DgCamera& cam, int space, double& z, double& w) {
    const double lin = cam.s * ((double)gs_quant16(pred) / 65535.0) + cam.t;
    z = space == DG_SPACE_DISPARITY ? 1.0 / lin : lin;
    w = 1.0 / z;
    return pred == pred && usable && dg_finite(z) && cam.z_min <= z && z <= cam.z_max;
}

// the view ray of pixel (u, v) without its 1
DG_HD void dg_ray(int u, int v, const DgCamera& cam, double& p0, double& p1) {
    p0 = ((double)u - cam.cx) / cam.fx;
    p1 = ((double)v - cam.cy) / cam.fy;
}

// Step 3, the sums of one pixel's window
struct DgSums {
    int n, su, sv, suu, suv, svv;
    double sw, suw, svw;
};

DG_HD void dg_sums_clear(DgSums& f) {
    f.n = f.su = f.sv = f.suu = f.suv = f.svv = 0;
    f.sw = f.suw = f.svw = 0.0;
}

// |z_j - z_i| <= lim with lim = tau * z_i; false for a NaN z_j
DG_HD bool dg_member(double zj, double zi, double lim) { return fabs(zj - zi) <= lim; }

DG_HD void dg_sums_add(DgSums& f, int du, int dv, double w) {
    f.n += 1, f.su += du, f.sv += dv, f.suu += du * du, f.suv += du * dv, f.svv += dv * dv;
    f.sw = f.sw + w;
    f.suw = f.suw + (double)du * w;
    f.svw = f.svw + (double)dv * w;
}

// the plane w = a du + b dv + c by the cofactors of the symmetric matrix, in the order of gs_solve; the determinant is returned
DG_HD double dg_solve(const DgSums& f, double& a, double& b, double& c) {
    const double s00 = (double)f.suu, s01 = (double)f.suv, s02 = (double)f.su, s11 = (double)f.svv, s12 = (double)f.sv, s22 = (double)f.n;
    const double c00 = s11 * s22 - s12 * s12;
    const double c01 = s02 * s12 - s01 * s22;
    const double c02 = s01 * s12 - s02 * s11;
    const double c11 = s00 * s22 - s02 * s02;
    const double c12 = s01 * s02 - s00 * s12;
    const double c22 = s00 * s11 - s01 * s01;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    a = ((c00 * f.suw + c01 * f.svw) + c02 * f.sw) / det;
    b = ((c01 * f.suw + c11 * f.svw) + c12 * f.sw) / det;
    c = ((c02 * f.suw + c12 * f.svw) + c22 * f.sw) / det;
    return det;
}

// Steps 2, 4 and 5 of pixel (u, v): valid and z from dg_depth, f the sums of its window (ignored for an invalid pixel).  xyz and nrm take the
// three float32 values each; returns whether the pixel is kept.
DG_HD bool dg_pixel(int u, int v, bool valid, double z, const DgSums& f, const DgCamera& cam, int min_count, double min_cos, float (&xyz)[3],
                    float (&nrm)[3]) {
    const double qnan = __builtin_nan("");
    double p0, p1;
    dg_ray(u, v, cam, p0, p1);
    xyz[0] = (float)(valid ? p0 * z : qnan);
    xyz[1] = (float)(valid ? p1 * z : qnan);
    xyz[2] = (float)(valid ? z : qnan);
    nrm[0] = nrm[1] = nrm[2] = 0.0f;
    if (!valid || f.n < min_count) return false;
    double a, b, c;
    const double det = dg_solve(f, a, b, c);
    if (!(det > 0.0)) return false;
    const double m0 = a * cam.fx, m1 = b * cam.fy, m2 = (c + a * (cam.cx - (double)u)) + b * (cam.cy - (double)v);
    const double mm = (m0 * m0 + m1 * m1) + m2 * m2;
    const double len = sqrt(mm);
    if (len > 0.0 && dg_finite(len)) {
        nrm[0] = (float)(-m0 / len);
        nrm[1] = (float)(-m1 / len);
        nrm[2] = (float)(-m2 / len);
    }
    const double mp = (m0 * p0 + m1 * p1) + m2;
    const double pp = (p0 * p0 + p1 * p1) + 1.0;
    return mp * mp >= ((min_cos * min_cos) * mm) * pp && mp > 0.0;
}
