"""numpy restatement of the training-label semantics (csrc/labels.hip) for sizes the fixture
tests/golden/labels_small.npz does not cover.  Test infrastructure: the CPU side of the bit-for-bit checks; pinned
itself against the reference's SK_Dataset / NU_Dataset outputs in tests/test_labels_cpu.py."""
import numpy as np

IGNORE = 255


def listed(sv2point, sv_flag, value, p):
    """bool [p]: the points at least one supervoxel with flag == value lists."""
    hit = np.zeros(p, dtype=bool)
    flags = np.asarray(sv_flag).astype(np.int64)
    for k in np.nonzero(flags == value)[0]:
        hit[np.asarray(sv2point[k], dtype=np.int64)] = True
    return hit


def train_labels(raw, label_map, sv2point=None, sv_flag=None, pseudo=None, unique_idxs=None):
    """raw u32 [P] (SemanticKITTI, class in the low half) or u8 [P] (nuScenes); label_map [260] / [100];
    sv2point a list of index arrays with sv_flag [S] in {0, 1, 2} (or both None: every point keeps its label);
    pseudo i64 [P] or None; unique_idxs i64 [N] or None.  Returns (labels_p i64 [P], labels_v i64 [N] or None)."""
    raw = np.asarray(raw)
    ids = (raw & 0xFFFF) if raw.dtype.itemsize == 4 else raw
    ids = ids.astype(np.int64)
    table = np.asarray(label_map).astype(np.int64)
    if ids.size and ids.max() >= table.shape[0]:
        raise IndexError('raw label id beyond the label table')
    labels_p = table[ids]
    if sv_flag is not None:
        labels_p = np.where(listed(sv2point, sv_flag, 1, ids.shape[0]), labels_p, IGNORE)
        if pseudo is not None:
            labels_p = np.where(listed(sv2point, sv_flag, 2, ids.shape[0]), np.asarray(pseudo, dtype=np.int64), labels_p)
    labels_p = labels_p.astype(np.int64)
    labels_v = labels_p[np.asarray(unique_idxs, dtype=np.int64)] if unique_idxs is not None else None
    return labels_p, labels_v
