// rmp2_hull.h -- nearest points of a convex hull and a point or segment (include/rmp2.h rmp2_set_link_hulls).
//
// The reference asks PyBullet for the closest points of a link's collision mesh -- loaded as its convex hull -- and an obstacle
// (simulation.py:462-484).  Here the hull is a vertex set plus outward face planes in the leaf's frame coordinates, the obstacle's
// axis (a sphere's centre, a capsule's segment) is brought into those coordinates, and GJK on the Minkowski difference
// hull - segment finds the nearest pair; an axis that meets the hull takes the separating face of least translation.
//
// Everything is fp64 (the vertex and plane data are fp32, exactly representable): the support function is an argmax over the
// hull's vertices and the stop test compares its value with |v|^2, both of which fp32 rounding would blur at the 1e-5 m the
// stage promises.  Every loop is bounded: at most kHullGjkIters GJK iterations (a pair that has not converged by then keeps
// the best simplex found), one pass over the vertices per support call, one pass over the planes for the face rule.
// Host-compilable (__host__ __device__) so that the same code can be exercised on the CPU.
#pragma once
#include <math.h>

namespace rmp2 {

constexpr int kHullGjkIters = 32;
constexpr double kHullTouch2 = 1e-14;   // |v|^2 below (1e-7 m)^2: the axis touches or meets the hull -> face rule

struct HullHit {
  double hp[3];   // nearest point of the hull (frame coordinates)
  double xp[3];   // the axis point c: the sphere centre, or the segment point GJK picks (the meeting endpoint x* under the face rule)
  double u[3];    // unit direction from c towards the hull point (-n_f* under the face rule)
  double gap;     // signed surface gap: |hp - c| - r outside, -(t_f* + r) when the axis meets the hull
  int iters;      // GJK iterations run (diagnostic)
};

__host__ __device__ inline double hdot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The non-finite contract (include/rmp2.h): 0 * x is 0 for every finite x and NaN for NaN and +-inf, so a sum of such products is
// NaN exactly when one input is not finite.  The routines below run on whatever they are given (every loop is bounded and every
// index stays in range with NaN comparisons false) and select NaN into each output field at the end: finite results keep their bits.
__host__ __device__ inline bool hull_poisoned(double zero_sum) { return !(zero_sum == 0.0); }
__host__ __device__ inline double hull_nan() { return __builtin_nan(""); }

// Closest point of conv(W[0..n)) to the origin, GJK's distance subalgorithm: lam = barycentric weights; the simplex is reduced
// in place to the smallest feature that holds the point.  Returns false when a full tetrahedron contains the origin.
struct HullSimplex {
  double W[4][3], H[4][3], S[4][3];
  int id[4];
  int n;
  double lam[4];
};

__host__ __device__ inline void hs_keep(HullSimplex& s, int k, const int* idx, const double* lam) {
  double W[4][3], H[4][3], S[4][3];
  int id[4];
  for (int i = 0; i < k; ++i)
    for (int c = 0; c < 3; ++c) W[i][c] = s.W[idx[i]][c], H[i][c] = s.H[idx[i]][c], S[i][c] = s.S[idx[i]][c];
  for (int i = 0; i < k; ++i) id[i] = s.id[idx[i]];
  for (int i = 0; i < k; ++i) {
    for (int c = 0; c < 3; ++c) s.W[i][c] = W[i][c], s.H[i][c] = H[i][c], s.S[i][c] = S[i][c];
    s.id[i] = id[i];
    s.lam[i] = lam[i];
  }
  s.n = k;
}

// segment i-j of the simplex: closest point to the origin as (which vertices, weights)
__host__ __device__ inline double hs_segment(const double A[3], const double B[3], int& k, double lam[2], int sel[2], int ia, int ib) {
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double den = hdot(ab, ab);
  const double t = den > 0.0 ? -hdot(A, ab) / den : 0.0;
  if (!(t > 0.0)) {
    k = 1, sel[0] = ia, lam[0] = 1.0;
    return hdot(A, A);
  }
  if (t >= 1.0) {
    k = 1, sel[0] = ib, lam[0] = 1.0;
    return hdot(B, B);
  }
  k = 2, sel[0] = ia, sel[1] = ib, lam[0] = 1.0 - t, lam[1] = t;
  const double p[3] = {A[0] + t * ab[0], A[1] + t * ab[1], A[2] + t * ab[2]};
  return hdot(p, p);
}

// triangle (Ericson, Real-Time Collision Detection 5.1.5, with the query point at the origin); a degenerate triangle falls back
// to the best of its three edges
__host__ __device__ inline double hs_triangle(const double A[3], const double B[3], const double C[3], int& k, double lam[3], int sel[3],
                                             int ia, int ib, int ic) {
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  const double ap[3] = {-A[0], -A[1], -A[2]};
  const double d1 = hdot(ab, ap), d2 = hdot(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) return k = 1, sel[0] = ia, lam[0] = 1.0, hdot(A, A);
  const double bp[3] = {-B[0], -B[1], -B[2]};
  const double d3 = hdot(ab, bp), d4 = hdot(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return k = 1, sel[0] = ib, lam[0] = 1.0, hdot(B, B);
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    int kk;
    double l2[2];
    int s2[2];
    const double r = hs_segment(A, B, kk, l2, s2, ia, ib);
    k = kk;
    for (int i = 0; i < kk; ++i) sel[i] = s2[i], lam[i] = l2[i];
    return r;
  }
  const double cp[3] = {-C[0], -C[1], -C[2]};
  const double d5 = hdot(ab, cp), d6 = hdot(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return k = 1, sel[0] = ic, lam[0] = 1.0, hdot(C, C);
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    int kk;
    double l2[2];
    int s2[2];
    const double r = hs_segment(A, C, kk, l2, s2, ia, ic);
    k = kk;
    for (int i = 0; i < kk; ++i) sel[i] = s2[i], lam[i] = l2[i];
    return r;
  }
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    int kk;
    double l2[2];
    int s2[2];
    const double r = hs_segment(B, C, kk, l2, s2, ib, ic);
    k = kk;
    for (int i = 0; i < kk; ++i) sel[i] = s2[i], lam[i] = l2[i];
    return r;
  }
  const double sum = va + vb + vc;
  if (!(sum > 0.0)) {   // degenerate (collinear) triangle: the best edge
    double best = 1e300;
    const double* P[3] = {A, B, C};
    const int I[3] = {ia, ib, ic};
    for (int e = 0; e < 3; ++e) {
      int kk;
      double l2[2];
      int s2[2];
      const double r = hs_segment(P[e], P[(e + 1) % 3], kk, l2, s2, I[e], I[(e + 1) % 3]);
      if (r < best) {
        best = r, k = kk;
        for (int i = 0; i < kk; ++i) sel[i] = s2[i], lam[i] = l2[i];
      }
    }
    return best;
  }
  const double v = vb / sum, w = vc / sum;
  k = 3, sel[0] = ia, sel[1] = ib, sel[2] = ic, lam[0] = 1.0 - v - w, lam[1] = v, lam[2] = w;
  const double p[3] = {A[0] + v * ab[0] + w * ac[0], A[1] + v * ab[1] + w * ac[1], A[2] + v * ab[2] + w * ac[2]};
  return hdot(p, p);
}

__host__ __device__ inline bool hs_solve(HullSimplex& s) {
  int k = 1, sel[3] = {0, 0, 0};
  double lam[3] = {1.0, 0.0, 0.0};
  if (s.n == 1) {
    s.lam[0] = 1.0;
    return true;
  }
  if (s.n == 2) {
    double l2[2];
    int s2[2];
    hs_segment(s.W[0], s.W[1], k, l2, s2, 0, 1);
    for (int i = 0; i < k; ++i) sel[i] = s2[i], lam[i] = l2[i];
  } else if (s.n == 3) {
    hs_triangle(s.W[0], s.W[1], s.W[2], k, lam, sel, 0, 1, 2);
  } else {
    // tetrahedron: the faces the origin lies outside of (opposite side from the fourth vertex; a flat tetrahedron counts every
    // face as such) -- none: the origin is inside
    const int F[4][4] = {{0, 1, 2, 3}, {0, 1, 3, 2}, {0, 2, 3, 1}, {1, 2, 3, 0}};
    double best = 1e300;
    bool any = false;
    for (int f = 0; f < 4; ++f) {
      const double* A = s.W[F[f][0]];
      const double* B = s.W[F[f][1]];
      const double* C = s.W[F[f][2]];
      const double* D = s.W[F[f][3]];
      const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
      const double nrm[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
      const double ad[3] = {D[0] - A[0], D[1] - A[1], D[2] - A[2]};
      const double so = -hdot(nrm, A), sd = hdot(nrm, ad);
      if (so * sd > 0.0) continue;   // origin on the fourth vertex's side of this face
      any = true;
      int kk, ss[3];
      double ll[3];
      const double r = hs_triangle(A, B, C, kk, ll, ss, F[f][0], F[f][1], F[f][2]);
      if (r < best) {
        best = r, k = kk;
        for (int i = 0; i < kk; ++i) sel[i] = ss[i], lam[i] = ll[i];
      }
    }
    if (!any) return false;
  }
  hs_keep(s, k, sel, lam);
  return true;
}

// The nearest points of the convex hull (V: nv vertices as float4 .xyz; Pl: nf planes (n, d), n . x <= d inside) and the
// segment a-b (a == b: a point) of radius r, all in the hull's coordinates.
__host__ __device__ inline HullHit hull_closest_finite(const float4* __restrict__ V, int nv, const float4* __restrict__ Pl, int nf,
                                                       const double a[3], const double b[3], double r) {
  HullHit out;
  HullSimplex s;
  const bool seg = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
  {
    const float4 v0 = V[0];
    const double h0[3] = {(double)v0.x, (double)v0.y, (double)v0.z};
    for (int c = 0; c < 3; ++c) s.H[0][c] = h0[c], s.S[0][c] = a[c], s.W[0][c] = h0[c] - a[c];
    s.id[0] = 0;
    s.n = 1;
    s.lam[0] = 1.0;
  }
  double v[3] = {s.W[0][0], s.W[0][1], s.W[0][2]};
  double vv = hdot(v, v);
  bool touch = false;
  int it = 0;
  for (; it < kHullGjkIters; ++it) {
    if (vv <= kHullTouch2) {
      touch = true;
      break;
    }
    // support of hull - segment in -v: the hull vertex maximising -v . x, the endpoint maximising v . x
    int jb = 0;
    double best = -1e300;
    for (int j = 0; j < nv; ++j) {
      const float4 q = V[j];
      const double d = -(v[0] * (double)q.x + v[1] * (double)q.y + v[2] * (double)q.z);
      if (d > best) best = d, jb = j;
    }
    const bool use_b = seg && hdot(v, b) > hdot(v, a);
    const double* e = use_b ? b : a;
    const int idw = 2 * jb + (use_b ? 1 : 0);
    bool dup = false;
    for (int i = 0; i < s.n; ++i) dup = dup || s.id[i] == idw;
    if (dup) break;
    const float4 q = V[jb];
    const double hw[3] = {(double)q.x, (double)q.y, (double)q.z};
    const double w[3] = {hw[0] - e[0], hw[1] - e[1], hw[2] - e[2]};
    if (vv - hdot(v, w) <= 1e-13 * vv) break;   // no vertex brings the difference measurably closer to the origin
    HullSimplex prev = s;
    for (int c = 0; c < 3; ++c) s.H[s.n][c] = hw[c], s.S[s.n][c] = e[c], s.W[s.n][c] = w[c];
    s.id[s.n] = idw;
    ++s.n;
    if (!hs_solve(s)) {   // a tetrahedron of the difference contains the origin: the axis meets the hull
      touch = true;
      break;
    }
    double nvv[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < s.n; ++i)
      for (int c = 0; c < 3; ++c) nvv[c] += s.lam[i] * s.W[i][c];
    const double nv2 = hdot(nvv, nvv);
    if (!(nv2 < vv)) {   // no progress (rounding): keep the previous simplex
      s = prev;
      break;
    }
    for (int c = 0; c < 3; ++c) v[c] = nvv[c];
    vv = nv2;
  }
  out.iters = it;
  if (!touch) {
    double hp[3] = {0.0, 0.0, 0.0}, xp[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < s.n; ++i)
      for (int c = 0; c < 3; ++c) hp[c] += s.lam[i] * s.H[i][c], xp[c] += s.lam[i] * s.S[i][c];
    const double d[3] = {hp[0] - xp[0], hp[1] - xp[1], hp[2] - xp[2]};
    const double dn = sqrt(hdot(d, d));
    if (dn * dn > kHullTouch2) {
      for (int c = 0; c < 3; ++c) out.hp[c] = hp[c], out.xp[c] = xp[c], out.u[c] = d[c] / dn;
      out.gap = dn - r;
      return out;
    }
  }
  // the axis meets (or touches) the hull: the face of least translation t_f = d_f - min over the endpoints of n_f . x
  int fb = 0;
  double tb = 1e300, mb = 0.0;
  bool at_b = false;
  for (int f = 0; f < nf; ++f) {
    const float4 p = Pl[f];
    const double n[3] = {(double)p.x, (double)p.y, (double)p.z};
    const double ma = hdot(n, a), mbb = hdot(n, b);
    const double m = mbb < ma ? mbb : ma;
    const double t = (double)p.w - m;
    if (t < tb) tb = t, fb = f, mb = m, at_b = mbb < ma;
  }
  (void)mb;
  const float4 p = Pl[fb];
  const double n[3] = {(double)p.x, (double)p.y, (double)p.z};
  const double* x = at_b ? b : a;
  for (int c = 0; c < 3; ++c) out.xp[c] = x[c], out.hp[c] = x[c] + tb * n[c], out.u[c] = -n[c];
  out.gap = -(tb + r);
  return out;
}

// A non-finite a, b or r: every field NaN (hull_poisoned).  Without it a NaN in b alone is never picked by the support test
// and the capsule is answered as the sphere at a, and a NaN in a falls through to the face rule's initial 1e300.
__host__ __device__ inline HullHit hull_closest(const float4* __restrict__ V, int nv, const float4* __restrict__ Pl, int nf,
                                                const double a[3], const double b[3], double r) {
  HullHit out = hull_closest_finite(V, nv, Pl, nf, a, b, r);
  const bool bad = hull_poisoned(0.0 * a[0] + 0.0 * a[1] + 0.0 * a[2] + 0.0 * b[0] + 0.0 * b[1] + 0.0 * b[2] + 0.0 * r);
  const double qn = hull_nan();
#pragma unroll
  for (int c = 0; c < 3; ++c) out.hp[c] = bad ? qn : out.hp[c], out.xp[c] = bad ? qn : out.xp[c], out.u[c] = bad ? qn : out.u[c];
  out.gap = bad ? qn : out.gap;
  return out;
}

// ---- two hulls (include/rmp2.h rmp2_set_self_collision_hulls) -------------------------------------------------------------
// The nearest points of hull A (vertices VA, planes PA, A's coordinates) and hull B (VB, PB, B's coordinates), B placed in A's
// coordinates by y = Rm y_B + t (Rm row-major).  GJK on the Minkowski difference A - B: B's support in direction d is taken in
// B's own coordinates against Rm^T d, so no vertex is transformed up front.  The simplex is kept as (vertex of A, vertex of B)
// index pairs plus weights and its points are re-read each step: a few registers instead of 36 doubles copied per iteration.
// Every array is indexed by unrolled constants or select chains, so the routine needs no scratch on the device.
// Overlapping or touching (|v|^2 <= kHullTouch2, or a tetrahedron that holds the origin): the face rule over the face normals
// n of A and the negated face normals of B, s(n) = min_{y in B} n . y - max_{x in A} n . x, n* = argmax s (A's faces first, the
// first maximum), y* the vertex of B attaining the min; p_b = y*, p_a = y* - s n*, gap = s < 0 (edge-edge axes are not weighed).
// Bounded: at most kPairGjkIters GJK steps (the best simplex found is kept), one pass over each hull's planes for the face rule.
constexpr int kPairGjkIters = 64;

struct PairHit {
  double pa[3];   // nearest point of A (A's coordinates): p_link
  double pb[3];   // nearest point of B (A's coordinates): p_obs
  double u[3];    // unit direction with pa - pb = gap u: from pb towards pa, -n* under the face rule
  double gap;     // signed: |pa - pb| apart, s(n*) < 0 under the face rule
  int iters;      // GJK iterations run (diagnostic)
  int face;       // 1: the face rule was taken
};

// index of the vertex maximising d . x (the first maximum)
__host__ __device__ inline int hull_support(const float4* __restrict__ V, int n, double d0, double d1, double d2) {
  int jb = 0;
  double best = -1e300;
  for (int j = 0; j < n; ++j) {
    const float4 q = V[j];
    const double s = d0 * (double)q.x + d1 * (double)q.y + d2 * (double)q.z;
    if (s > best) best = s, jb = j;
  }
  return jb;
}

// A's vertex ja and B's vertex jb, both in A's coordinates
__host__ __device__ inline void pair_points(const float4* __restrict__ VA, const float4* __restrict__ VB, const double Rm[9],
                                            const double t[3], int ja, int jb, double x[3], double y[3]) {
  const float4 a = VA[ja], b = VB[jb];
  x[0] = a.x, x[1] = a.y, x[2] = a.z;
#pragma unroll
  for (int i = 0; i < 3; ++i) y[i] = Rm[3 * i] * (double)b.x + Rm[3 * i + 1] * (double)b.y + Rm[3 * i + 2] * (double)b.z + t[i];
}

__host__ __device__ inline int pick4(const int a[4], int i) { return i == 0 ? a[0] : i == 1 ? a[1] : i == 2 ? a[2] : a[3]; }

// segment A-B: closest point to the origin; always writes sel[0..1], lam[0..1]
__host__ __device__ inline double pg_segment(const double A[3], const double B[3], int ia, int ib, int& k, int sel[2], double lam[2]) {
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]};
  const double den = hdot(ab, ab);
  const double t = den > 0.0 ? -hdot(A, ab) / den : 0.0;
  if (!(t > 0.0)) return k = 1, sel[0] = ia, sel[1] = ia, lam[0] = 1.0, lam[1] = 0.0, hdot(A, A);
  if (t >= 1.0) return k = 1, sel[0] = ib, sel[1] = ib, lam[0] = 1.0, lam[1] = 0.0, hdot(B, B);
  k = 2, sel[0] = ia, sel[1] = ib, lam[0] = 1.0 - t, lam[1] = t;
  const double p[3] = {A[0] + t * ab[0], A[1] + t * ab[1], A[2] + t * ab[2]};
  return hdot(p, p);
}

// triangle (hs_triangle's regions); always writes sel[0..2], lam[0..2]
__host__ __device__ inline double pg_triangle(const double A[3], const double B[3], const double C[3], int ia, int ib, int ic, int& k,
                                              int sel[3], double lam[3]) {
  sel[2] = ia, lam[2] = 0.0;
  const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
  const double ap[3] = {-A[0], -A[1], -A[2]};
  const double d1 = hdot(ab, ap), d2 = hdot(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) return k = 1, sel[0] = sel[1] = ia, lam[0] = 1.0, lam[1] = 0.0, hdot(A, A);
  const double bp[3] = {-B[0], -B[1], -B[2]};
  const double d3 = hdot(ab, bp), d4 = hdot(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) return k = 1, sel[0] = sel[1] = ib, lam[0] = 1.0, lam[1] = 0.0, hdot(B, B);
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) return pg_segment(A, B, ia, ib, k, sel, lam);
  const double cp[3] = {-C[0], -C[1], -C[2]};
  const double d5 = hdot(ab, cp), d6 = hdot(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) return k = 1, sel[0] = sel[1] = ic, lam[0] = 1.0, lam[1] = 0.0, hdot(C, C);
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) return pg_segment(A, C, ia, ic, k, sel, lam);
  const double va = d3 * d6 - d5 * d4;
  if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) return pg_segment(B, C, ib, ic, k, sel, lam);
  const double sum = va + vb + vc;
  if (!(sum > 0.0)) {   // degenerate (collinear) triangle: the best edge
    int k1, k2, k3, s1[2], s2[2], s3[2];
    double l1[2], l2[2], l3[2];
    const double r1 = pg_segment(A, B, ia, ib, k1, s1, l1), r2 = pg_segment(B, C, ib, ic, k2, s2, l2), r3 = pg_segment(C, A, ic, ia, k3, s3, l3);
    const bool b2 = r2 < r1 && r2 <= r3, b3 = !b2 && r3 < r1;
    k = b2 ? k2 : b3 ? k3 : k1;
    sel[0] = b2 ? s2[0] : b3 ? s3[0] : s1[0], sel[1] = b2 ? s2[1] : b3 ? s3[1] : s1[1];
    lam[0] = b2 ? l2[0] : b3 ? l3[0] : l1[0], lam[1] = b2 ? l2[1] : b3 ? l3[1] : l1[1];
    return b2 ? r2 : b3 ? r3 : r1;
  }
  const double v = vb / sum, w = vc / sum;
  k = 3, sel[0] = ia, sel[1] = ib, sel[2] = ic, lam[0] = 1.0 - v - w, lam[1] = v, lam[2] = w;
  const double p[3] = {A[0] + v * ab[0] + w * ac[0], A[1] + v * ab[1] + w * ac[1], A[2] + v * ab[2] + w * ac[2]};
  return hdot(p, p);
}

// GJK's distance subalgorithm on the n (1..4) points W: the smallest feature holding the closest point, as k slots sel[0..k) of W
// with weights lam.  False when the tetrahedron contains the origin.
__host__ __device__ inline bool pg_solve(const double W[4][3], int n, int& k, int sel[3], double lam[3]) {
  sel[0] = sel[1] = sel[2] = 0, lam[0] = 1.0, lam[1] = lam[2] = 0.0, k = 1;
  if (n == 1) return true;
  if (n == 2) {
    pg_segment(W[0], W[1], 0, 1, k, sel, lam);
    return true;
  }
  if (n == 3) {
    pg_triangle(W[0], W[1], W[2], 0, 1, 2, k, sel, lam);
    return true;
  }
  // tetrahedron: the faces the origin lies outside of (hs_solve's test); none: the origin is inside
  double best = 1e300;
  bool any = false;
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int i0 = f == 3 ? 1 : 0, i1 = f <= 1 ? 1 : 2, i2 = f == 0 ? 2 : 3, i3 = f == 0 ? 3 : f == 1 ? 2 : f == 2 ? 1 : 0;
    const double* A = W[i0];
    const double* B = W[i1];
    const double* C = W[i2];
    const double* D = W[i3];
    const double ab[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, ac[3] = {C[0] - A[0], C[1] - A[1], C[2] - A[2]};
    const double nrm[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
    const double ad[3] = {D[0] - A[0], D[1] - A[1], D[2] - A[2]};
    const double so = -hdot(nrm, A), sd = hdot(nrm, ad);
    if (so * sd > 0.0) continue;
    any = true;
    int kk, ss[3];
    double ll[3];
    const double r = pg_triangle(A, B, C, i0, i1, i2, kk, ss, ll);
    if (r < best) {
      best = r, k = kk;
      sel[0] = ss[0], sel[1] = ss[1], sel[2] = ss[2], lam[0] = ll[0], lam[1] = ll[1], lam[2] = ll[2];
    }
  }
  return any;
}

__host__ __device__ inline PairHit hull_pair_closest_finite(const float4* __restrict__ VA, int na, const float4* __restrict__ PA, int fa,
                                                            const float4* __restrict__ VB, int nb, const float4* __restrict__ PB, int fb,
                                                            const double Rm[9], const double t[3]) {
  PairHit out;
  int ia[4] = {0, 0, 0, 0}, ib[4] = {0, 0, 0, 0};
  double lam[4] = {1.0, 0.0, 0.0, 0.0};
  int n = 1;
  double v[3];
  {
    double x[3], y[3];
    pair_points(VA, VB, Rm, t, 0, 0, x, y);
    v[0] = x[0] - y[0], v[1] = x[1] - y[1], v[2] = x[2] - y[2];
  }
  double vv = hdot(v, v);
  bool touch = false;
  int it = 0;
  for (; it < kPairGjkIters; ++it) {
    if (vv <= kHullTouch2) {
      touch = true;
      break;
    }
    // support of A - B in -v: A's vertex maximising -v . x, B's vertex maximising v . y = (Rm^T v) . y_B
    const int ja = hull_support(VA, na, -v[0], -v[1], -v[2]);
    const int jb = hull_support(VB, nb, Rm[0] * v[0] + Rm[3] * v[1] + Rm[6] * v[2], Rm[1] * v[0] + Rm[4] * v[1] + Rm[7] * v[2],
                                Rm[2] * v[0] + Rm[5] * v[1] + Rm[8] * v[2]);
    bool dup = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) dup = dup || (i < n && ia[i] == ja && ib[i] == jb);
    if (dup) break;
    double x[3], y[3];
    pair_points(VA, VB, Rm, t, ja, jb, x, y);
    const double w[3] = {x[0] - y[0], x[1] - y[1], x[2] - y[2]};
    if (vv - hdot(v, w) <= 1e-13 * vv) break;   // no vertex pair brings the difference measurably closer to the origin
    int pia[4], pib[4];
    double plam[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) pia[i] = ia[i], pib[i] = ib[i], plam[i] = lam[i];
    const int pn = n;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i == n) ia[i] = ja, ib[i] = jb;
    ++n;
    double W[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double xi[3], yi[3];
      pair_points(VA, VB, Rm, t, i < n ? ia[i] : 0, i < n ? ib[i] : 0, xi, yi);
#pragma unroll
      for (int c = 0; c < 3; ++c) W[i][c] = xi[c] - yi[c];
    }
    int k, sel[3];
    double l3[3];
    if (!pg_solve(W, n, k, sel, l3)) {   // a tetrahedron of the difference contains the origin: the hulls overlap
      touch = true;
      break;
    }
    double nvv[3] = {0.0, 0.0, 0.0};
    int nia[4], nib[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int si = sel[i];
      nia[i] = pick4(ia, si), nib[i] = pick4(ib, si);
      const double li = i < k ? l3[i] : 0.0;
#pragma unroll
      for (int c = 0; c < 3; ++c) nvv[c] += li * (si == 0 ? W[0][c] : si == 1 ? W[1][c] : si == 2 ? W[2][c] : W[3][c]);
    }
    const double nv2 = hdot(nvv, nvv);
    if (!(nv2 < vv)) {   // no progress (rounding): keep the previous simplex
#pragma unroll
      for (int i = 0; i < 4; ++i) ia[i] = pia[i], ib[i] = pib[i], lam[i] = plam[i];
      n = pn;
      break;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) ia[i] = nia[i], ib[i] = nib[i], lam[i] = i < k ? l3[i] : 0.0;
    lam[3] = 0.0;
    n = k;
    v[0] = nvv[0], v[1] = nvv[1], v[2] = nvv[2];
    vv = nv2;
  }
  out.iters = it;
  out.face = 0;
  if (!touch) {
    double pa[3] = {0.0, 0.0, 0.0}, pb[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= n) continue;
      double x[3], y[3];
      pair_points(VA, VB, Rm, t, ia[i], ib[i], x, y);
#pragma unroll
      for (int c = 0; c < 3; ++c) pa[c] += lam[i] * x[c], pb[c] += lam[i] * y[c];
    }
    const double d[3] = {pa[0] - pb[0], pa[1] - pb[1], pa[2] - pb[2]};
    const double dn = sqrt(hdot(d, d));
    if (dn * dn > kHullTouch2) {
#pragma unroll
      for (int c = 0; c < 3; ++c) out.pa[c] = pa[c], out.pb[c] = pb[c], out.u[c] = d[c] / dn;
      out.gap = dn;
      return out;
    }
  }
  // the hulls overlap (or touch): the face rule
  double best = -1e300;
  int side = 0, fbest = 0;
  for (int f = 0; f < fa; ++f) {   // A's faces: s = min_y n . y - d_f, min_y n . y = min_{y_B} (Rm^T n) . y_B + n . t
    const float4 p = PA[f];
    const double nn[3] = {(double)p.x, (double)p.y, (double)p.z};
    const double m0 = Rm[0] * nn[0] + Rm[3] * nn[1] + Rm[6] * nn[2], m1 = Rm[1] * nn[0] + Rm[4] * nn[1] + Rm[7] * nn[2],
                 m2 = Rm[2] * nn[0] + Rm[5] * nn[1] + Rm[8] * nn[2];
    double mn = 1e300;
    for (int j = 0; j < nb; ++j) {
      const float4 q = VB[j];
      const double s = m0 * (double)q.x + m1 * (double)q.y + m2 * (double)q.z;
      mn = s < mn ? s : mn;
    }
    const double s = mn + hdot(nn, t) - (double)p.w;
    if (s > best) best = s, side = 0, fbest = f;
  }
  for (int g = 0; g < fb; ++g) {   // B's faces, n = -Rm m: s = -d_m - (Rm m) . t + min_x (Rm m) . x
    const float4 p = PB[g];
    const double rm[3] = {Rm[0] * p.x + Rm[1] * p.y + Rm[2] * p.z, Rm[3] * p.x + Rm[4] * p.y + Rm[5] * p.z,
                          Rm[6] * p.x + Rm[7] * p.y + Rm[8] * p.z};
    double mn = 1e300;
    for (int j = 0; j < na; ++j) {
      const float4 q = VA[j];
      const double s = rm[0] * (double)q.x + rm[1] * (double)q.y + rm[2] * (double)q.z;
      mn = s < mn ? s : mn;
    }
    const double s = -(double)p.w - hdot(rm, t) + mn;
    if (s > best) best = s, side = 1, fbest = g;
  }
  double ns[3];
  if (side == 0) {
    const float4 p = PA[fbest];
    ns[0] = p.x, ns[1] = p.y, ns[2] = p.z;
  } else {
    const float4 p = PB[fbest];
    ns[0] = -(Rm[0] * p.x + Rm[1] * p.y + Rm[2] * p.z), ns[1] = -(Rm[3] * p.x + Rm[4] * p.y + Rm[5] * p.z),
    ns[2] = -(Rm[6] * p.x + Rm[7] * p.y + Rm[8] * p.z);
  }
  // y*: B's vertex minimising n* . y, i.e. maximising -(Rm^T n*) . y_B
  const int js = hull_support(VB, nb, -(Rm[0] * ns[0] + Rm[3] * ns[1] + Rm[6] * ns[2]), -(Rm[1] * ns[0] + Rm[4] * ns[1] + Rm[7] * ns[2]),
                              -(Rm[2] * ns[0] + Rm[5] * ns[1] + Rm[8] * ns[2]));
  double x[3], y[3];
  pair_points(VA, VB, Rm, t, 0, js, x, y);
#pragma unroll
  for (int c = 0; c < 3; ++c) out.pb[c] = y[c], out.pa[c] = y[c] - best * ns[c], out.u[c] = -ns[c];
  out.gap = best;
  out.face = 1;
  return out;
}

// A non-finite entry of Rm or t: every real field NaN (hull_poisoned; iters and face are diagnostics and stay).
__host__ __device__ inline PairHit hull_pair_closest(const float4* __restrict__ VA, int na, const float4* __restrict__ PA, int fa,
                                                     const float4* __restrict__ VB, int nb, const float4* __restrict__ PB, int fb,
                                                     const double Rm[9], const double t[3]) {
  PairHit out = hull_pair_closest_finite(VA, na, PA, fa, VB, nb, PB, fb, Rm, t);
  double z = 0.0 * t[0] + 0.0 * t[1] + 0.0 * t[2];
#pragma unroll
  for (int i = 0; i < 9; ++i) z += 0.0 * Rm[i];
  const bool bad = hull_poisoned(z);
  const double qn = hull_nan();
#pragma unroll
  for (int c = 0; c < 3; ++c) out.pa[c] = bad ? qn : out.pa[c], out.pb[c] = bad ? qn : out.pb[c], out.u[c] = bad ? qn : out.u[c];
  out.gap = bad ? qn : out.gap;
  return out;
}

}  // namespace rmp2
