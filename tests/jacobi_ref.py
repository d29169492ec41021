"""Restatement of csrc/sym3.h, the cyclic Jacobi that the surface variation and the VCCS normals share (used by
redal_ref.py and vccs_ref.py).  Python floats throughout: every product and sum is rounded on its own, as in the kernels."""
import math


def jacobi3(a):
    """a: 3x3 list (symmetric), changed in place: at most 32 sweeps of the rotations (0,1), (0,2), (1,2).  Leaves the
    eigenvalues on a's diagonal and returns e, whose columns are the eigenvectors."""
    e = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]

    def rot(p, q):
        apq = a[p][q]
        if apq == 0.0:
            return
        theta = (a[q][q] - a[p][p]) / (2.0 * apq)
        t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
        cs = 1.0 / math.sqrt(t * t + 1.0)
        s = t * cs
        r = 3 - p - q
        arp, arq = a[r][p], a[r][q]
        a[r][p] = a[p][r] = cs * arp - s * arq
        a[r][q] = a[q][r] = s * arp + cs * arq
        a[p][p] -= t * apq
        a[q][q] += t * apq
        a[p][q] = a[q][p] = 0.0
        for i in range(3):
            ep, eq = e[i][p], e[i][q]
            e[i][p] = cs * ep - s * eq
            e[i][q] = s * ep + cs * eq

    for _ in range(32):
        off = abs(a[0][1]) + abs(a[0][2]) + abs(a[1][2])
        dia = abs(a[0][0]) + abs(a[1][1]) + abs(a[2][2])
        if not (off > 1e-300) or off <= 1e-18 * dia:
            break
        rot(0, 1)
        rot(0, 2)
        rot(1, 2)
    return e
