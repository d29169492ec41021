"""Greedy active / pseudo-label selection (counterpart of
/root/reference/score/sv_level/LiDAL.py:225-325).  Deliberately host-side Python on numpy
arrays with the SAME constructs as the reference (np.argsort order, iteration over a Python
`set`, first-hit break): the outcome depends on CPython's set iteration order, so
a re-ordered or parallel version could not reproduce the reference's flags.

Two passes share one routine:
  AL  (flag 1): unlabeled supervoxels by DESCENDING divergence; a candidate within 5 m of an
      already added one replaces it only if its entropy is HIGHER.
  SL  (flag 2): candidates are the supervoxels still unlabeled after AL *before* old flag-2s are
      reset (so last round's pseudo labels are not re-picked), ASCENDING divergence, zeros
      skipped; replacement only if entropy is LOWER.
Each pass stops when 1 % of `train_point_num` points has been spent.

`select` evaluates the distance of a candidate to every added supervoxel, O(visited x added) small numpy calls.
Which supervoxels lie within the radius of each other does not depend on any order: `centre_pairs` computes that
table once, on the GPU (csrc/neighbours.hip), and `select_indexed` runs the same two passes on it, going back to the
real `set` only to learn which of several hits comes first.
"""
import numpy as np

__all__ = ['select', 'select_indexed', 'centre_pairs']


def _greedy_pass(order, cand_ids, cand_div, flags, label, prefer_higher_entropy, skip_zero,
                 sv_interes, sv_pnums, sv_centers, budget, radius):
    added = set()
    for idx in order:
        if skip_zero and cand_div[idx] == 0:
            continue
        sv = cand_ids[idx]
        centre = sv_centers[sv]
        free = True
        for other in added:
            dist = np.sqrt(np.square(centre - sv_centers[other]).sum())
            if dist < radius:
                free = False
                wins = (sv_interes[other] < sv_interes[sv] if prefer_higher_entropy
                        else sv_interes[other] > sv_interes[sv])
                if wins:
                    flags[sv] = label
                    flags[other] = 0
                    added.add(sv)
                    added.remove(other)
                    budget = budget + sv_pnums[other] - sv_pnums[sv]
                break
        if free:
            budget -= sv_pnums[sv]
            if budget < 0:
                break
            flags[sv] = label
            added.add(sv)
    return flags


def select(sv_flags, sv_interds, sv_interes, sv_pnums, sv_centers, train_point_num,
           sv_dis_thresh=5.0):
    flags = np.array(sv_flags).astype(int)
    cand = np.where(flags == 0)[0]
    div = sv_interds[cand]
    order = np.argsort(div)
    flags = _greedy_pass(reversed(order), cand, div, flags, 1, True, False, sv_interes, sv_pnums,
                         sv_centers, round(0.01 * train_point_num), sv_dis_thresh)
    cand = np.where(flags == 0)[0]
    div = sv_interds[cand]
    order = np.argsort(div)
    flags[flags == 2] = 0
    flags = _greedy_pass(order, cand, div, flags, 2, False, True, sv_interes, sv_pnums,
                         sv_centers, round(0.01 * train_point_num), sv_dis_thresh)
    return flags


def centre_pairs(sv_centers, radius=5.0):
    """The table of all pairs of centres within `radius` of each other, computed on the device (lidal_radius_pairs_count
    / _fill, csrc/neighbours.hip): (row_ptr i64 [n + 1], col i32 [pairs]) as host numpy arrays; row i = every j != i,
    ascending, for which `np.sqrt(np.square(sv_centers[i] - sv_centers[j]).sum()) < radius` is true in f32, bit for bit.
    A centre with a NaN or infinite coordinate has an empty row and is in no row (numpy's compare is false there).

    sv_centers: f32 [n, 3], a numpy array or a CUDA tensor; anything else is a TypeError.  It depends on the centres
    alone, which a dataset computes once (sv_centers.npy): one table serves both passes and every later round.
    A radius that float32 cannot hold exactly is refused: the reference compares an f32 distance with the Python float,
    and whether that compare runs in f32 or f64 depends on the numpy version's promotion rules."""
    import torch

    from .. import backend as B
    on_host = isinstance(sv_centers, np.ndarray)
    if not on_host and not (torch.is_tensor(sv_centers) and sv_centers.is_cuda):
        raise TypeError('centre_pairs: sv_centers must be a numpy array or a CUDA tensor, float32 [n, 3]')
    if sv_centers.dtype != (np.float32 if on_host else torch.float32) or sv_centers.ndim != 2 or sv_centers.shape[1] != 3:
        raise TypeError('centre_pairs: sv_centers must be float32 [n, 3], got %s %s'
                        % (sv_centers.dtype, tuple(sv_centers.shape)))
    radius = float(radius)
    with np.errstate(over='ignore'):
        r32 = float(np.float32(radius))
    if not (0.0 < radius < float('inf')) or r32 != radius:
        raise ValueError('centre_pairs: the radius must be positive, finite and exact in float32 (got %r): for any '
                         'other the reference\'s compare depends on numpy\'s promotion rules' % radius)
    c = torch.from_numpy(np.ascontiguousarray(sv_centers)).cuda() if on_host else sv_centers.contiguous()
    B.require_gpu(c)
    n, dev = c.shape[0], c.device
    row_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    nbytes = B.lib().lidal_radius_pairs_workspace_bytes(n)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_radius_pairs_count(B.ptr(c), n, radius, B.ptr(row_ptr), B.ptr(status), B.ptr(ws), nbytes,
                                             B.stream()), 'radius_pairs_count')
    row_ptr_host = row_ptr.cpu().numpy()                # the one synchronisation between the two calls
    if int(status.item()) != 0:
        raise ValueError('centre_pairs: a centre lies outside the search grid (2^20 - 1 cells of the smallest power '
                         'of two >= %g on either side of the origin)' % radius)
    col = torch.empty(int(row_ptr_host[n]), dtype=torch.int32, device=dev)
    B.check(B.lib().lidal_radius_pairs_fill(B.ptr(c), n, radius, B.ptr(row_ptr), B.ptr(col), B.ptr(ws), nbytes,
                                            B.stream()), 'radius_pairs_fill')
    return row_ptr_host, col.cpu().numpy()


def _greedy_pass_indexed(order, cand_ids, cand_div, flags, label, prefer_higher_entropy, skip_zero,
                         sv_interes, sv_pnums, row_ptr, col, budget, stats):
    added = set()                                       # the reference's set, with the reference's add / remove sequence
    is_added = np.zeros(flags.shape[0], dtype=bool)     # the same membership, indexable by a row of the table
    for idx in order:
        if skip_zero and cand_div[idx] == 0:
            continue
        sv = cand_ids[idx]
        row = col[row_ptr[sv]:row_ptr[sv + 1]]
        hits = row[is_added[row]]
        if hits.size == 0:
            stats['free'] += 1
            budget -= sv_pnums[sv]
            if budget < 0:
                break
            flags[sv] = label
            added.add(sv)
            is_added[sv] = True
            continue
        if hits.size == 1:
            stats['one_hit'] += 1
            other = hits[0]
        else:                                           # which hit the reference's loop meets first: ask the set itself
            stats['multi_hit'] += 1
            hit_set = set(hits.tolist())
            for other in added:
                if other in hit_set:
                    break
        wins = (sv_interes[other] < sv_interes[sv] if prefer_higher_entropy
                else sv_interes[other] > sv_interes[sv])
        if wins:
            flags[sv] = label
            flags[other] = 0
            added.add(sv)
            added.remove(other)
            is_added[sv] = True
            is_added[other] = False
            budget = budget + sv_pnums[other] - sv_pnums[sv]
    return flags


def select_indexed(sv_flags, sv_interds, sv_interes, sv_pnums, sv_centers, train_point_num,
                   sv_dis_thresh=5.0, pairs=None, details=False):
    """`select` with the distance loop replaced by a look-up in the table of `centre_pairs`: the same flags, bit for
    bit, at every size.

    pairs: (row_ptr, col) of the centres within sv_dis_thresh of each other, from `centre_pairs` (None: it is called
    here) or from anywhere else that states the reference's expression; one table serves both passes and later rounds.
    details=True returns (flags, counts), counts = how many candidates met no / one / several added neighbours.

    Why the flags are equal.  The reference walks `for other in added:` and stops at the first member whose distance
    to the candidate is below the radius.  Whether a member is such a hit is a fixed, symmetric, order-free fact of
    sv_centers: it is row `sv` of the table.  So
      * no member of the row is added: the walk finds nothing, the free branch;
      * one is: the walk ends at that member, wherever in the set it stands;
      * several are: the first depends on the set's iteration order, so the walk is made, over the REAL
        set, comparing membership in the row in place of distances.  That set has received exactly the add / remove
        sequence the reference's would have: the same values (a set places its members by their hash, and an integer
        hashes alike whatever its width) in the same order, hence the same table history and the same iteration order.
    Everything after the hit (entropy compare, flags, budget) is the reference's code unchanged.  A candidate is never
    its own hit: it is visited once and added only by its own visit."""
    flags = np.array(sv_flags).astype(int)
    if pairs is None:
        pairs = centre_pairs(sv_centers, sv_dis_thresh)
    row_ptr, col = np.asarray(pairs[0]), np.asarray(pairs[1])
    if row_ptr.shape != (flags.shape[0] + 1,):
        raise ValueError('select_indexed: the table has %d rows, the board %d supervoxels'
                         % (row_ptr.shape[0] - 1, flags.shape[0]))
    stats = [{'free': 0, 'one_hit': 0, 'multi_hit': 0} for _ in range(2)]
    cand = np.where(flags == 0)[0]
    div = sv_interds[cand]
    order = np.argsort(div)
    flags = _greedy_pass_indexed(reversed(order), cand, div, flags, 1, True, False, sv_interes, sv_pnums,
                                 row_ptr, col, round(0.01 * train_point_num), stats[0])
    cand = np.where(flags == 0)[0]
    div = sv_interds[cand]
    order = np.argsort(div)
    flags[flags == 2] = 0
    flags = _greedy_pass_indexed(order, cand, div, flags, 2, False, True, sv_interes, sv_pnums,
                                 row_ptr, col, round(0.01 * train_point_num), stats[1])
    if details:
        return flags, {k: stats[0][k] + stats[1][k] for k in stats[0]}
    return flags
