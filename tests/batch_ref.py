"""numpy restatement of the one-sort batch voxelisation (lidal_voxelize_batch).  TEST
INFRASTRUCTURE: the per-point arithmetic is oracle.voxelize_ref's lines, the batch is ONE stable sort of
sample << 39 | x << 26 | y << 13 | z over all points followed by run heads; `per_scan` is the formulation it must equal:
oracle.voxelize_ref.voxelize_scan per sample and the reference's collate rule (sk_dataset.py:188-242)."""
import numpy as np

from oracle import voxelize_ref


def point_coords(points, intensity, trans_m, rnd, scale=20, full_scale=8192):
    """voxelize_ref.voxelize_scan up to astype(int): (coords_v int64 [P,3], feats_p f32 [P,4], all points valid)."""
    raw = np.concatenate([points, intensity[:, None]], axis=1).astype(np.float32)
    feats_p = np.zeros_like(raw)
    feats_p[:, 3] = raw[:, 3]
    coords_p = np.matmul(raw[:, :3], trans_m)
    feats_p[:, :3] = coords_p
    coords_p = coords_p * scale
    if len(coords_p) == 0:
        return np.zeros((0, 3), dtype=np.int64), feats_p, True
    full = np.array([full_scale] * 3)
    cmin, cmax = coords_p.min(0), coords_p.max(0)
    offset = (-cmin + np.clip(full - cmax + cmin - 0.001, 0, None) * rnd[:3]
              + np.clip(full - cmax + cmin + 0.001, None, 0) * rnd[3:])
    coords_p = coords_p + offset
    valid = (coords_p.min(1) >= 0) * (coords_p.max(1) < full_scale)
    return coords_p.astype(int).astype(np.int64), feats_p, bool(valid.all())


def one_sort(samples, scale=20, full_scale=8192):
    """samples: list of (points f32 [P,3], intensity f32 [P], trans_m, rnd).  Returns the dict of data.voxelize_batch on
    the host (coords_v_b int32 [N,4], feats_v_b, inverse_indices_b, unique_idxs_b, voxel_ptr, point_ptr)."""
    keys, feats = [], []
    for s, (pts, inten, m, rnd) in enumerate(samples):
        c, f, ok = point_coords(pts, inten, np.asarray(m), np.asarray(rnd), scale, full_scale)
        assert ok, 'input voxels are not valid: sample %d' % s
        keys.append((s << 39) | (c[:, 0] << 26) | (c[:, 1] << 13) | c[:, 2])
        feats.append(f)
    keys, feats = np.concatenate(keys), np.concatenate(feats)
    n_samples = len(samples)
    point_ptr = np.concatenate([[0], np.cumsum([len(x[0]) for x in samples])]).astype(np.int64)
    order = np.argsort(keys, kind='stable')
    skeys = keys[order]
    head = np.ones(len(skeys), dtype=bool)
    head[1:] = skeys[1:] != skeys[:-1]
    run = np.cumsum(head) - 1                                   # the run number of every sorted point
    inverse = np.empty(len(keys), dtype=np.int64)
    inverse[order] = run
    hk = skeys[head]
    coords = np.stack([(hk >> 26) & 0x1FFF, (hk >> 13) & 0x1FFF, hk & 0x1FFF, hk >> 39], 1).astype(np.int32)
    uniq = order[head].astype(np.int64)                         # stable: the first point of a run is the smallest row
    voxel_ptr = np.searchsorted(hk >> 39, np.arange(n_samples + 1)).astype(np.int64)
    return {'coords_v_b': coords, 'feats_v_b': feats[uniq], 'inverse_indices_b': inverse, 'unique_idxs_b': uniq,
            'voxel_ptr': voxel_ptr, 'point_ptr': point_ptr}


def per_scan(samples, scale=20, full_scale=8192):
    """voxelize_ref.voxelize_scan per sample + collate_fn: the same dict."""
    coords, feats, inverse, uniq, voxel_ptr, point_ptr = [], [], [], [], [0], [0]
    for s, (pts, inten, m, rnd) in enumerate(samples):
        if len(pts) == 0:
            cv, fv = np.zeros((0, 3), dtype=np.int64), np.zeros((0, 4), dtype=np.float32)
            ui = inv = np.zeros(0, dtype=np.int64)
        else:
            cv, fv, ui, inv = voxelize_ref.voxelize_scan(pts, inten, np.asarray(m), np.asarray(rnd), scale, full_scale)
        coords.append(np.concatenate([cv, np.full((len(cv), 1), s)], 1).astype(np.int32))
        feats.append(fv)
        inverse.append(inv.astype(np.int64) + voxel_ptr[-1])     # collate_fn: + the voxels of the samples before
        uniq.append(ui.astype(np.int64) + point_ptr[-1])
        voxel_ptr.append(voxel_ptr[-1] + len(cv))
        point_ptr.append(point_ptr[-1] + len(pts))
    return {'coords_v_b': np.concatenate(coords), 'feats_v_b': np.concatenate(feats),
            'inverse_indices_b': np.concatenate(inverse), 'unique_idxs_b': np.concatenate(uniq),
            'voxel_ptr': np.array(voxel_ptr, dtype=np.int64), 'point_ptr': np.array(point_ptr, dtype=np.int64)}


# ---- the shapes of the tests (seeded, shared by the CPU and the GPU file) -------------------------------------------------
def box_points(rng, n):
    """n points uniform in a 100 x 100 x 6 m box, and intensities."""
    pts = (rng.random((n, 3)) * np.array([100.0, 100.0, 6.0]) - np.array([50.0, 50.0, 3.0])).astype(np.float32)
    return pts, rng.random(n).astype(np.float32)


def draws(seed, n):
    from lidal_amd import data
    rs = np.random.RandomState(seed)
    return [data.draw_augmentation(rs) for _ in range(n)]


def box_samples(sizes, seed):
    rng = np.random.default_rng(seed)
    return [box_points(rng, n) + d for n, d in zip(sizes, draws(seed, len(sizes)))]


def view_samples(n_points, n_views, seed):
    pts, inten = box_points(np.random.default_rng(seed), n_points)
    return [(pts, inten) + d for d in draws(seed, n_views)]


def duplicate_samples(seed, n_samples=3, n_points=600, n_distinct=3):
    rng = np.random.default_rng(seed)
    out = []
    for d in draws(seed, n_samples):
        pts, inten = box_points(rng, n_distinct)
        pick = rng.integers(0, n_distinct, n_points)
        out.append((pts[pick], inten[pick]) + d)
    return out


def field_end_samples():
    """Two samples of 64 points: x and y run over 0 .. 409.59 m, z alternates between 0 and 409.59; identity matrix and
    all draws 0.5, so the offset is 0 and the voxel indices 0 and 8191 occur in every axis."""
    out = []
    for s in range(2):
        t = np.linspace(0.0, 409.59, 64)
        x, y = (t, t[::-1]) if s == 0 else (t[::-1], t)
        z = np.where(np.arange(64) % 2 == 0, 0.0, 409.59)
        pts = np.stack([x, y, z], 1).astype(np.float32)
        out.append((pts, np.linspace(0, 1, 64).astype(np.float32), np.eye(3), np.full(6, 0.5)))
    return out


SIZES = {'one': [1], 'n257': [257], 'borders': [255, 256, 257, 1], 'empty': [0, 300, 0], 'many': [40] * 32}
