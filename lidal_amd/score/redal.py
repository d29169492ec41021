"""ReDAL region selection on the GPU: the baseline that the reference ships next to LiDAL
(the reference's score/sv_level/ReDAL.py, with its curvature input dataset/ReDAL/gen_surface_variation_sk.py).

  surface_variation / knn   gen_surface_variation_sk.py::boundary_extractor: k = 50 nearest other points of every
                            point of a raw scan, sigma = lambda_min / (lambda_1 + lambda_2 + lambda_3) of their
                            covariance, clipped at 0.1 (lidal_surface_variation, lidal_knn)
  region_scores             ReDAL.py::worker_func for one frame: per-point uncertainty + curvature score, then per
                            supervoxel the mean score, the mean [96] feature and the point count (lidal_region_scores)
  kmeans                    the sklearn.cluster.KMeans(150, random_state=0) of ReDAL.py:220-223, as this project
                            defines it (greedy k-means++ + Lloyd; lidal_kmeans)
  select_redal              ReDAL.py:199-247 in host numpy, the reference's own constructs
  RegionBoard               the global per-region arrays of ReDAL.py:152-190 and the scatter by sv_id
  redal_sequence            infer_frame(return_feat=True) -> surface variation -> region scores per frame

A note on the curvature definition: pyntcloud 0.1.5, which the reference uses, is not available to this project, so
what it computes is recalled, not read.  As recalled, `get_neighbors(k=50)` is a KD-tree query of k + 1 with the
first column (the point itself) dropped, and the eigenvalues (named e1(51)..e3(51)) are those of the covariance of the
50 neighbours WITHOUT the query point.  That is the definition implemented here, with the population covariance (the
normalisation cancels in the ratio) in f64 and Jacobi eigenvalues; pyntcloud itself works in f32 with LAPACK, whose last
bits are not a goal.
"""
import numpy as np
import torch

from .. import backend as B

__all__ = ['surface_variation', 'knn', 'region_scores', 'kmeans', 'select_redal', 'RegionBoard', 'redal_sequence',
           'KNN_CELL', 'FT_DIM']

FT_DIM = 96            # ReDAL.py:22
KNN_CELL = 0.5         # search grid cell (metres); the neighbours do not depend on it, only the search time does


GRID_CELLS = 2 ** 20 - 1        # csrc/grid.h: cell indices beyond +-GRID_CELLS are outside the grid's key range


def _xyz(xyz, cell):
    if not torch.is_tensor(xyz):
        xyz = torch.from_numpy(np.ascontiguousarray(xyz, dtype=np.float32)).cuda()
    B.require_gpu(xyz)
    xyz = xyz.float().contiguous()
    assert xyz.ndim == 2 and xyz.shape[1] == 3, tuple(xyz.shape)
    if xyz.shape[0] == 0:
        return xyz
    reach = float(xyz.abs().max())          # (NaN if any coordinate is; the one synchronisation of this check)
    if not reach < float('inf'):
        # a NaN query never fills its list and searches until its ring covers the scan's cell box
        raise ValueError('knn / surface_variation: the coordinates must be finite (NaN or inf found)')
    if not reach < (GRID_CELLS - 1) * float(cell):
        # the grid build parks such a point in a cell no query forms a key for: the search would silently miss it
        raise ValueError('knn / surface_variation: a coordinate of magnitude %g is outside the search grid '
                         '(%d cells of %g)' % (reach, GRID_CELLS, float(cell)))
    return xyz


def knn(xyz, k, cell=KNN_CELL):
    """The k nearest OTHER points of every point of xyz (f32 [P,3]): i32 [P,k] device tensor, sorted by distance, ties
    to the lower index.  P < k + 1 raises (the reference would index out of range)."""
    xyz = _xyz(xyz, cell)
    p = xyz.shape[0]
    out = torch.empty((p, k), dtype=torch.int32, device=xyz.device)
    nbytes = B.lib().lidal_knn_workspace_bytes(p)
    ws = B.workspace(nbytes, xyz.device)
    B.check(B.lib().lidal_knn(B.ptr(xyz), p, int(k), float(cell), B.ptr(out), B.ptr(ws), nbytes, B.stream()), 'knn')
    return out


def surface_variation(xyz, k=50, threshold=0.1, cell=KNN_CELL):
    """gen_surface_variation_sk.py::boundary_extractor(xyz, threshold=0.1) with k_n = 50: f32 [P] device tensor.
    threshold=None leaves sigma unclipped."""
    xyz = _xyz(xyz, cell)
    p = xyz.shape[0]
    out = torch.empty(p, dtype=torch.float32, device=xyz.device)
    nbytes = B.lib().lidal_knn_workspace_bytes(p)
    ws = B.workspace(nbytes, xyz.device)
    thr = float('inf') if threshold is None else float(threshold)
    B.check(B.lib().lidal_surface_variation(B.ptr(xyz), p, int(k), float(cell), thr, B.ptr(out), B.ptr(ws), nbytes,
                                            B.stream()), 'surface_variation')
    return out


def region_scores(prob, feat, curvature, sv_ptr, sv_idx, alpha=1.0, gamma=0.05):
    """ReDAL.py::worker_func for one frame, on device tensors: prob f32 [P,C], feat f32 [P,D] (the `outfeat` of
    infer_frame(return_feat=True)), curvature f32 [P], and the supervoxel CSR of interframe.sv_csr.
    Returns (sv_scores f32 [S], sv_feats f32 [S,D], sv_pnums i64 [S]) device tensors."""
    B.require_gpu(prob, feat, curvature, sv_ptr, sv_idx)
    prob = prob.float().contiguous()
    feat = feat.float().contiguous()
    curvature = curvature.float().contiguous()
    sv_ptr = sv_ptr.to(torch.int64).contiguous()
    sv_idx = sv_idx.to(torch.int64).contiguous()
    p, c = prob.shape
    d = feat.shape[1]
    assert feat.shape[0] == p and curvature.shape == (p,), (tuple(feat.shape), tuple(curvature.shape), p)
    s = sv_ptr.numel() - 1
    dev = prob.device
    sv_scores = torch.empty(s, dtype=torch.float32, device=dev)
    sv_feats = torch.empty((s, d), dtype=torch.float32, device=dev)
    sv_pnums = torch.empty(s, dtype=torch.int64, device=dev)
    nbytes = B.lib().lidal_region_scores_workspace_bytes(p)
    ws = B.workspace(nbytes, dev)
    B.check(B.lib().lidal_region_scores(B.ptr(prob), p, c, B.ptr(feat), d, B.ptr(curvature), B.ptr(sv_ptr),
                                        B.ptr(sv_idx), s, float(alpha), float(gamma), B.ptr(sv_scores),
                                        B.ptr(sv_feats), B.ptr(sv_pnums), B.ptr(ws), nbytes, B.stream()),
            'region_scores')
    return sv_scores, sv_feats, sv_pnums


def kmeans_draws(n, n_clusters, seed):
    """The host random draws of one restart: (first row, u f64 [k-1, trials]) from numpy.random.RandomState(seed) in
    the order greedy k-means++ consumes them (randint(n), then random_sample(trials) per further centre)."""
    trials = 2 + int(np.log(n_clusters))
    rs = np.random.RandomState(seed)
    first = int(rs.randint(n))
    u = np.stack([rs.random_sample(trials) for _ in range(n_clusters - 1)]) if n_clusters > 1 else \
        np.zeros((0, trials))
    return first, u.astype(np.float64), trials


def kmeans_single(x, n_clusters, seed, max_iter=300, tol=0.0):
    """One restart (the RandomState(seed) stream); tol is absolute.  Returns (labels i32 [N], centers f64 [k,D],
    inertia, n_iter, seeds i32 [k]); tensors on the device."""
    B.require_gpu(x)
    x = x.float().contiguous()
    n, d = x.shape
    if not 1 <= n_clusters <= n:
        raise ValueError('kmeans: n_clusters=%d must be in 1..n_samples=%d' % (n_clusters, n))
    first, u, trials = kmeans_draws(n, n_clusters, seed)
    dev = x.device
    u_dev = torch.from_numpy(u.reshape(-1).copy() if u.size else np.zeros(1)).to(dev)
    seeds = torch.empty(n_clusters, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    centers = torch.empty((n_clusters, d), dtype=torch.float64, device=dev)
    inertia = np.zeros(1, dtype=np.float64)
    n_iter = np.zeros(1, dtype=np.int32)
    nbytes = B.lib().lidal_kmeans_workspace_bytes(n, d, n_clusters, trials)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    B.check(B.lib().lidal_kmeans(B.ptr(x), n, d, n_clusters, first, B.ptr(u_dev), trials, int(max_iter), float(tol),
                                 B.ptr(seeds), B.ptr(labels), B.ptr(centers), inertia.ctypes.data, n_iter.ctypes.data,
                                 B.ptr(ws), nbytes, B.stream()), 'kmeans')
    return labels, centers, float(inertia[0]), int(n_iter[0]), seeds


def kmeans(x, n_clusters=150, random_state=0, n_init=10, max_iter=300, tol=1e-4):
    """k-means of the rows of x (f32 [N,D], D <= 128; a device tensor or a numpy array) in place of
    sklearn.cluster.KMeans(n_clusters, random_state=random_state).fit(x): n_init restarts with the seeds
    RandomState(random_state).randint(2**31 - 1, size=n_init), greedy k-means++ seeding, Lloyd iterations until the
    labels stop changing or the summed squared centre shift is <= tol * mean(var(x, axis=0)).  The restart of least
    inertia wins (the first on ties).  Returns (labels i64 [N] numpy, centers f64 [k,D] numpy, inertia, n_iter)."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B.require_gpu(x)
    x = x.float().contiguous()
    n = x.shape[0]
    if not 1 <= n_clusters <= n:
        raise ValueError('kmeans: n_clusters=%d must be in 1..n_samples=%d' % (n_clusters, n))
    tol_abs = float(torch.var(x.double(), dim=0, unbiased=False).mean().item()) * tol
    seeds = np.random.RandomState(random_state).randint(2 ** 31 - 1, size=n_init)
    best = None
    for s in seeds:
        labels, centers, inertia, n_iter, _ = kmeans_single(x, n_clusters, int(s), max_iter, tol_abs)
        if best is None or inertia < best[2]:
            best = (labels, centers, inertia, n_iter)
    labels, centers, inertia, n_iter = best
    return labels.cpu().numpy().astype(np.int64), centers.cpu().numpy(), inertia, n_iter


def select_redal(sv_flags, sv_scores, sv_feats, sv_pnums, train_point_num, trim_rate=0.1, num_clusters=150,
                 decay_rate=0.95, labels=None):
    """ReDAL.py:199-247: the diversity-aware selection over all regions.  sv_flags: the current flags (0 = unlabeled);
    returns the new flags (int, {0, 1} where the input was {0, 1}).  labels: the cluster of each of the top
    trim_rate share of unlabeled regions (by score, descending); None runs `kmeans` on their features on the GPU."""
    sv_flags = np.asarray(sv_flags).astype(int)
    sv_scores = np.asarray(sv_scores)
    sv_pnums = np.asarray(sv_pnums)
    unlabeled_ids = np.where(sv_flags == 0)[0]
    unlabeled_scores = sv_scores[unlabeled_ids]
    # sorted (first time)
    sorted_ids = np.argsort(unlabeled_scores)[::-1]
    unlabeled_ids_sorted = unlabeled_ids[sorted_ids]
    unlabeled_scores_sorted = unlabeled_scores[sorted_ids]
    N = int(unlabeled_ids_sorted.shape[0] * trim_rate)
    unlabeled_scores_sorted = unlabeled_scores_sorted[:N]
    unlabeled_ids_sorted = unlabeled_ids_sorted[:N]
    if labels is None:
        feats = np.asarray(sv_feats)[unlabeled_ids_sorted]
        labels, _, _, _ = kmeans(feats, n_clusters=num_clusters, random_state=0)
    clusters = np.asarray(labels)
    assert clusters.shape == (N,), (clusters.shape, N)
    # importance re-weighting
    importance_arr = [1 for _ in range(num_clusters)]
    for i in range(N):
        cluster_i = clusters[i]
        cluster_importance = importance_arr[cluster_i]
        unlabeled_scores_sorted[i] *= cluster_importance
        importance_arr[cluster_i] *= decay_rate
    # sorted (second time)
    sorted_ids = np.argsort(unlabeled_scores_sorted)[::-1]
    unlabeled_ids_sorted = unlabeled_ids_sorted[sorted_ids]
    point_limit = round(0.01 * train_point_num)
    for sv_id in unlabeled_ids_sorted:
        point_limit -= sv_pnums[sv_id]
        if point_limit < 0:
            break
        sv_flags[sv_id] = 1
    return sv_flags


class RegionBoard:
    """The global per-region arrays of ReDAL.py:152-163 (scores, features, point counts) and the scatter of each
    frame's results into them by sv_id (:176-190).  sv_pnums: the cached counts of an earlier round
    (super_voxel/VCCS/sv_pnums.npy, the reference's `sv_pre`), which are then kept."""

    def __init__(self, n_sv, sv_pnums=None, ft_dim=FT_DIM):
        self.sv_scores = np.zeros(n_sv, dtype=np.float32)
        self.sv_feats = np.zeros((n_sv, ft_dim), dtype=np.float32)
        self.sv_pre = sv_pnums is not None
        self.sv_pnums = np.asarray(sv_pnums) if self.sv_pre else np.zeros(n_sv, dtype=int)

    def add(self, sv_id, sv_scores, sv_feats, sv_pnums=None):
        sv_id = np.asarray(sv_id)
        self.sv_scores[sv_id] = _host(sv_scores)
        self.sv_feats[sv_id] = _host(sv_feats)
        if not self.sv_pre and sv_pnums is not None:
            self.sv_pnums[sv_id] = _host(sv_pnums)

    def add_sequence(self, sv_ids, results):
        """results: redal_sequence()'s list, sv_ids: per frame the global ids (the pickle's sv_id)."""
        for ids, (sc, ft, pn) in zip(sv_ids, results):
            self.add(ids, sc, ft, pn)

    def select(self, sv_flags, train_point_num, labels=None, **kw):
        return select_redal(sv_flags, self.sv_scores, self.sv_feats, self.sv_pnums, train_point_num, labels=labels,
                            **kw)


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def redal_sequence(model, frames, inf_reps=8, autocast=False, alpha=1.0, gamma=0.05, k=50, threshold=0.1):
    """ReDAL's scoring pass over one sequence on one GPU: per frame infer_frame(return_feat=True) (prob_inference.py
    with `outfeat`), the curvature (frame['curvature'], f32 [P] as loaded by io.load_curvature, or surface_variation
    of frame['points'], the raw scan f32 [P,3]), then region_scores.  Frame dicts are score_sequence's (coords, feats,
    inverse, sv_ptr, sv_idx; `world` is not read) plus `points` or `curvature`.  Only S x 98 numbers per frame stay
    resident: returns per frame (sv_scores f32 [S], sv_feats f32 [S,96], sv_pnums i64 [S]) device tensors."""
    from .prob_inference import infer_frame
    out = []
    for d in frames:
        prob, _, feat = infer_frame(model, d['coords'], d['feats'], d['inverse'], inf_reps, autocast=autocast,
                                    return_feat=True)
        if d.get('curvature') is not None:
            curv = d['curvature']
            if not torch.is_tensor(curv):
                curv = torch.from_numpy(np.asarray(curv, dtype=np.float32))
            curv = curv.to(prob.device)
        else:
            curv = surface_variation(d['points'], k=k, threshold=threshold)
        out.append(region_scores(prob, feat, curv, d['sv_ptr'], d['sv_idx'], alpha, gamma))
    return out
