// The 3x3 symmetric eigenproblem of a point neighbourhood, one copy for the units that must round it the same way
// (redal.hip: the surface variation of the k nearest neighbours; vccs.hip: the normal of a voxel's two-ring).  f64, every
// product and sum rounded on its own (-ffp-contract=off, lidal_amd/build.py); restated by tests/jacobi_ref.py.
#pragma once

#include "common.h"

namespace lidal {
namespace sym3 {

// Mean and population covariance of n members.  each(visit) calls visit(x, y, z) once per member, in the members' order;
// it runs twice: for the mean (summed in order, times 1 / n), then for the six second moments about it (times 1 / n).
template <class Each>
__device__ __forceinline__ void covariance3(Each each, int n, double (&a)[3][3]) {
  double mx = 0.0, my = 0.0, mz = 0.0;
  each([&](double x, double y, double z) { mx += x; my += y; mz += z; });
  const double inv = 1.0 / (double)n;
  mx *= inv; my *= inv; mz *= inv;
  double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
  each([&](double x, double y, double z) {
    const double dx = x - mx, dy = y - my, dz = z - mz;
    a00 += dx * dx; a01 += dx * dy; a02 += dx * dz;
    a11 += dy * dy; a12 += dy * dz; a22 += dz * dz;
  });
  a[0][0] = a00 * inv; a[0][1] = a[1][0] = a01 * inv; a[0][2] = a[2][0] = a02 * inv;
  a[1][1] = a11 * inv; a[1][2] = a[2][1] = a12 * inv; a[2][2] = a22 * inv;
}

// Cyclic Jacobi on the symmetric a: at most 32 sweeps of the rotations (0,1), (0,2), (1,2), until the off-diagonal mass
// is nothing (<= 1e-300) or at most 1e-18 of the diagonal's; the eigenvalues are left on a's diagonal.  Jacobi keeps
// the small eigenvalue of a nearly planar neighbourhood to ~1 ulp of the large ones (the closed trigonometric form
// loses it to cancellation).  VECTORS: e, the identity on entry, takes the same rotations (columns = eigenvectors).
template <bool VECTORS>
__device__ __forceinline__ void jacobi3(double (&a)[3][3], double (&e)[3][3]) {
  auto rot = [&](int P, int Q) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const int r = 3 - P - Q;
    const double arp = a[r][P], arq = a[r][Q];
    a[r][P] = a[P][r] = c * arp - s * arq;
    a[r][Q] = a[Q][r] = s * arp + c * arq;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    if (VECTORS) {
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double ep = e[i][P], eq = e[i][Q];
        e[i][P] = c * ep - s * eq;
        e[i][Q] = s * ep + c * eq;
      }
    }
  };
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]);
    const double dia = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
    if (!(off > 1e-300) || off <= 1e-18 * dia) break;
    rot(0, 1);
    rot(0, 2);
    rot(1, 2);
  }
}

}  // namespace sym3
}  // namespace lidal
