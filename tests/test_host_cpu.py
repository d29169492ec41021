"""CPU tests of the shipped package's host logic: the C-ABI library loads and exports every
symbol include/lidal_amd.h declares, operators refuse CPU tensors (no fallback), containers /
modules / model definitions keep the reference's surface, selection matches the reference's
flags, synthetic inputs follow the reference's input contract."""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from lidal_amd import backend as B
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    declared = set(re.findall(r'\b(lidal_[a-z0-9_]+)\s*\(', header))
    assert len(declared) >= 29
    handle = ctypes.CDLL(B.LIB_PATH)
    for name in declared:
        assert hasattr(handle, name), name
    assert declared == set(B.SIGNATURES), declared ^ set(B.SIGNATURES)
    assert B.lib().lidal_version() >= 100
    assert B.lib().lidal_hash_table_bytes(1000) == 2048 * 13 + 16384 + 64       # slots + hashed bitmap, spatial bitmap, header (csrc/common.h)
    assert B.lib().lidal_last_error() is not None


def test_plan_operation_kinds_match_the_header_and_the_prototypes():
    """The launch plans (lidal_plan_run): lidal_amd/network/plan.py's operation kinds are the header's enum, and
    every kind takes exactly the arguments of the entry point it stands for (prototype minus the stream); a plan
    with an unknown kind or a truncated operation is refused before anything is launched (no GPU needed)."""
    import array
    from lidal_amd import backend as B
    from lidal_amd.network import plan
    header = open(os.path.join(ROOT, 'include', 'lidal_amd.h')).read()
    enum = dict((k, int(v)) for k, v in re.findall(r'LIDAL_OP_([A-Z0-9_]+) = (\d+)', header))
    assert len(enum) >= 27
    mine = {k[3:]: v for k, v in vars(plan).items() if k.startswith('OP_') and isinstance(v, int)}
    assert mine == enum
    L = B.lib()
    protos = {}
    for m in re.finditer(r'\b(?:int|int64_t)\s+lidal_([a-z0-9_]+)\s*\(([^)]*)\)\s*;', header):
        protos[m.group(1)] = len([a for a in m.group(2).split(',') if a.strip() and a.strip() != 'void'])
    for name, kind in enum.items():
        n = L.lidal_plan_op_args(kind)
        if name in ('FORK_SIDE', 'JOIN_SIDE'):
            assert n == 0
        else:
            assert n == protos[name.lower()] - 1, (name, n, protos[name.lower()])
            assert n == len(B.SIGNATURES['lidal_' + name.lower()][1]) - 1
    assert L.lidal_plan_op_args(0) == -1 and L.lidal_plan_op_args(999) == -1
    bad = array.array('q', [999, 0, 0])
    assert L.lidal_plan_run(bad.buffer_info()[0], 3, 1, None, None) != 0
    assert b'unknown kind' in L.lidal_last_error()
    short = array.array('q', [plan.OP_COPY2D, 0, 0])
    assert L.lidal_plan_run(short.buffer_info()[0], 3, 1, None, None) != 0
    assert b'truncated' in L.lidal_last_error()
    empty = array.array('q', [0])
    assert L.lidal_plan_run(empty.buffer_info()[0], 0, 0, None, None) == 0


def test_operators_have_no_cpu_fallback():
    from lidal_amd.nn import functional as F
    c = torch.zeros((4, 4), dtype=torch.int)
    for call in (lambda: F.sphash(c),
                 lambda: F.sphashquery(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int64)),
                 lambda: F.spcount(torch.zeros(3, dtype=torch.int), 2),
                 lambda: F.spvoxelize(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int), torch.ones(2, dtype=torch.int)),
                 lambda: F.spdevoxelize(torch.zeros(3, 4), torch.zeros((3, 8), dtype=torch.int), torch.zeros(3, 8)),
                 lambda: F.spdownsample(c),
                 lambda: F.build_kernel_map(c, (1, 1, 1), (3, 3, 3), (1, 1, 1))):
        with pytest.raises(RuntimeError, match='GPU only'):
            call()
    import lidal_amd
    with pytest.raises(RuntimeError, match='GPU only'):
        F.conv3d(lidal_amd.SparseTensor(torch.zeros(4, 4), c), torch.zeros(27, 4, 8), 3)


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'lidal_amd')):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', src, re.M), os.path.join(dirpath, f)


def test_containers_and_modules_surface():
    import lidal_amd
    import lidal_amd.nn as spnn
    from lidal_amd.nn.utils import get_kernel_offsets
    x = lidal_amd.SparseTensor(torch.ones(3, 2), torch.zeros((3, 4), dtype=torch.int), 2)
    assert x.s == (2, 2, 2) and x.F is x.feats and x.C is x.coords
    y = x + x
    assert y.cmaps is x.cmaps and y.kmaps is x.kmaps and torch.equal(y.F, 2 * x.F)
    x.F = torch.zeros(3, 5)
    assert x.feats.shape == (3, 5)
    z = lidal_amd.PointTensor(torch.ones(3, 2), torch.zeros(3, 4))
    assert z.idx_query == {} and z.additional_features == {'idx_query': {}, 'counts': {}}
    assert lidal_amd.cat([y, y]).F.shape == (3, 4)
    conv = spnn.Conv3d(4, 8, kernel_size=3)
    assert tuple(conv.kernel.shape) == (27, 4, 8) and conv.bias is None
    assert conv.kernel.abs().max() <= 1 / (4 * 27) ** 0.5
    assert tuple(spnn.Conv3d(4, 8, kernel_size=1).kernel.shape) == (4, 8)
    assert tuple(spnn.Conv3d(8, 4, kernel_size=2, stride=2, transposed=True).kernel.shape) == (8, 8, 4)
    assert isinstance(spnn.BatchNorm(8), torch.nn.BatchNorm1d)
    assert get_kernel_offsets(2, (2, 2, 2)).dtype == torch.int


def test_models_keep_reference_state_dict_surface(golden_dir):
    from lidal_amd.network import SPVCNN, MinkUNet
    from weights import fill_state_dict, state_dict_signature
    for name, cls, n_params in (('spvcnn', SPVCNN, 21778003), ('minkunet', MinkUNet, 21723315)):
        model = cls(19)
        assert sum(p.numel() for p in model.parameters()) == n_params
        ref = json.load(open(os.path.join(golden_dir, 'state_dict_%s.json' % name)))
        assert [[k, list(s), d] for k, s, d in state_dict_signature(model)] == ref
        fill_state_dict(model)      # strict=True load of a reference-shaped checkpoint


def test_selection_matches_reference_flags(golden_dir):
    from lidal_amd.score import select
    g = np.load(os.path.join(golden_dir, 'selection_small.npz'))
    out = select(g['flags_in'], g['sv_interds'], g['sv_interes'], g['sv_pnums'], g['sv_centers'],
                 int(g['train_point_num']))
    assert np.array_equal(out, g['flags_out'])
    # budget branch (never binding with the reference's hard-coded 2.3e9 points): a tiny budget
    # must stop each pass early and still agree with the oracle restatement
    from oracle import scoring_ref
    small = int(g['sv_pnums'][:40].sum() * 100)
    a = select(g['flags_in'], g['sv_interds'], g['sv_interes'], g['sv_pnums'], g['sv_centers'], small)
    b = scoring_ref.select(g['flags_in'], g['sv_interds'], g['sv_interes'], g['sv_pnums'],
                           g['sv_centers'], small)
    assert np.array_equal(a, b) and 0 < (a == 1).sum() < (out == 1).sum()


def test_neighbour_ids_match_oracle():
    from lidal_amd.score import neighbour_ids
    from oracle import scoring_ref
    for n_frames, nei in ((25, 24), (40, 24), (30, 10), (11, 10)):
        for i in range(n_frames):
            assert neighbour_ids(i, n_frames, nei) == scoring_ref.neighbour_ids(i, n_frames, nei)


def test_synthetic_inputs_follow_reference_contract():
    from lidal_amd import synth
    b = synth.make_train_batch(n_frames=2, n_points=3000, seed=1)
    c, f, l = b['coords_v_b'], b['feats_v_b'], b['labels_v_b']
    assert c.dtype == np.int32 and c.shape[1] == 4 and f.dtype == np.float32 and f.shape[1] == 4
    assert l.dtype == np.int64 and set(np.unique(l)) <= set(range(19)) | {255}
    assert c[:, :3].min() >= 0 and c[:, :3].max() < 8192 and set(np.unique(c[:, 3])) == {0, 1}
    for bi in (0, 1):                               # np.unique(axis=0): sorted, distinct rows
        rows = c[c[:, 3] == bi, :3]
        assert len(np.unique(rows, axis=0)) == len(rows)
        assert np.array_equal(rows, rows[np.lexsort(rows.T[::-1])])
    rng = np.random.default_rng(0)
    pts, inten = synth.raycast_scan(synth.make_world(2), (15.0, 0.0), rng, n_beams=16, n_az=64)
    sb = synth.make_score_batch(pts, inten, rng, inf_reps=3)
    inv = sb['inverse_indices_b']
    assert inv.shape[0] == 3 * pts.shape[0] and inv.max() == sb['coords_v_b'].shape[0] - 1
    seq = synth.make_sequence(3, n_points=500, seed=2, n_beams=8, n_az=128)
    assert seq[1]['world'].dtype == np.float64 and len(seq[1]['sv2point']) == 20
    assert sorted(np.concatenate(seq[1]['sv2point']).tolist()) == list(range(500))


def test_on_disk_formats_round_trip_and_match_reference_layout(tmp_path, golden_dir):
    """files written by lidal_amd.io have the reference's dtypes/shapes/pickle layout,
    and a reference-format checkpoint (DDP 'module.' prefix included) loads strict=True."""
    import pickle
    from lidal_amd import io as lio
    from lidal_amd.network import MinkUNet
    prob = torch.rand(50, 19)
    pred = prob.argmax(1)
    lio.save_prob_pred(str(tmp_path / 'prob/000001.npy'), str(tmp_path / 'pred/000001.npy'), prob, pred)
    p = np.load(tmp_path / 'prob/000001.npy')
    assert p.dtype == np.float32 and p.shape == (50, 19)
    assert np.load(tmp_path / 'pred/000001.npy').dtype == np.int64
    assert torch.equal(lio.load_prob(str(tmp_path / 'prob/000001.npy')), prob)
    sv_id = np.arange(40, 60, dtype=np.int64)
    sv2point = [np.arange(i, 50, 20, dtype=np.int64) for i in range(20)]
    lio.save_supervoxels(str(tmp_path / 'sv/000001.pickle'), sv_id, sv2point)
    with open(tmp_path / 'sv/000001.pickle', 'rb') as f:          # as LiDAL.py:84-85 reads it
        a, b = pickle.load(f)
    assert np.array_equal(a, sv_id) and all(np.array_equal(x, y) for x, y in zip(b, sv2point))
    sid, s2p = lio.load_supervoxels(str(tmp_path / 'sv/000001.pickle'))
    assert np.array_equal(sid, sv_id) and len(s2p) == 20
    lio.save_sv_flag(str(tmp_path / 'flag/000001.npy'), np.array([0, 1, 2] * 6 + [0, 0]))
    assert set(lio.load_sv_flag(str(tmp_path / 'flag/000001.npy')).tolist()) == {0, 1, 2}
    model = MinkUNet(19)
    lio.save_checkpoint(str(tmp_path / 'ckpt'), model, 500, 3)
    raw = torch.load(tmp_path / 'ckpt/current.pt')
    assert set(raw) == {'model_state_dict', 'iteration', 'ep_id'}
    ref_keys = [k for k, _, _ in json.load(open(os.path.join(golden_dir, 'state_dict_minkunet.json')))]
    assert list(raw['model_state_dict']) == ref_keys
    torch.save({'model_state_dict': {'module.' + k: v for k, v in raw['model_state_dict'].items()},
                'iteration': 7, 'ep_id': 1}, tmp_path / 'ddp.pt')
    assert lio.load_checkpoint(str(tmp_path / 'ddp.pt'), MinkUNet(19)) == (7, 1)


def test_iou_from_confusion_matches_reference_formula():
    from lidal_amd.evaluate import iou_from_confusion
    rng = np.random.default_rng(0)
    conf = rng.integers(0, 1000, (19, 19)).astype(np.int32)
    conf[:, 5] = 0
    conf[5, :] = 0                                    # a class never seen: IoU is nan as in iou_sk
    ious, miou = iou_from_confusion(conf)
    for i in range(19):
        tp = conf[i, i]; fp = conf[i].sum() - tp; fn = conf[:, i].sum() - tp
        if tp + fp + fn == 0:
            assert np.isnan(ious[i])
        else:
            assert ious[i] == tp / (tp + fp + fn)
    assert np.isnan(miou)


def test_wgrad_scratch_plan_is_bounded_and_occupancy_sized():
    """lidal_conv_wgrad_slabs (host arithmetic, no GPU): the bf16 DMA kernel asks for one slab per
    workgroup of ONE resident round (<= 512) + k, and fewer when the rows would leave a workgroup
    less than ~16 stages; the split-K register kernels ask for <= 256 slabs per offset."""
    from lidal_amd import backend as B
    slabs = B.lib().lidal_conv_wgrad_slabs
    for n in (1, 500, 17000, 105000, 397000, 3000000):
        for ca, cb in ((32, 32), (96, 96), (128, 96), (256, 256), (384, 256)):
            for k in (1, 8, 27):
                assert k + 1 <= slabs(n, n, k, ca, cb, 1) <= 512 + k          # bf16
                assert k <= slabs(n, n, k, ca, cb, 0) <= 256 * k              # f32
    assert slabs(397000, 397000, 27, 96, 96, 1) == 256 + 27          # line-bound level 0: one per CU
    assert slabs(397000, 397000, 27, 32, 32, 1) == 512 + 27          # small stages: two per CU
    assert slabs(43000, 43000, 27, 256, 256, 1) == 128 + 27          # four channel tiles share the round
    assert slabs(1000, 1000, 27, 96, 96, 1) < 16 + 27                # a small level: few, long enough runs
    assert slabs(397000, 397000, 27, 100, 96, 1) == slabs(397000, 397000, 27, 100, 96, 1)
    assert slabs(397000, 397000, 27, 100, 96, 1) % 27 == 0           # 100 channels: the split-K kernel


def test_io_reads_files_the_reference_wrote(tmp_path, golden_dir):
    """tests/golden/io_small.npz holds the BYTES of files from the
    Processing_files tree of make_golden.py's selection run -- sv_flag of round 1, sv_pnums.npy and
    sv_centers.npy were written by the reference's own __main__ (LiDAL.py:220-222,328-330), the
    prob map / supervoxel pickle / round-0 flags are the inputs it consumed -- next to the arrays
    they decode to.  lidal_amd.io must read each of them, and what it writes must read back the
    same through the loaders the reference uses (np.load / pickle.load)."""
    import pickle
    from lidal_amd import io as lio
    g = np.load(os.path.join(golden_dir, 'io_small.npz'))

    def put(name, key):
        p = tmp_path / name
        p.write_bytes(g[key].tobytes())
        return str(p)
    f1 = lio.load_sv_flag(put('flag1.npy', 'file_sv_flag_1r'))
    assert f1.dtype == np.int64 and np.array_equal(f1, g['sv_flag_1r']) and set(f1.tolist()) <= {0, 1, 2}
    assert np.array_equal(lio.load_sv_flag(put('flag0.npy', 'file_sv_flag_0r')), g['sv_flag_0r'])
    pn, ce = lio.load_sv_stats(put('sv_pnums.npy', 'file_sv_pnums'), put('sv_centers.npy', 'file_sv_centers'))
    assert pn.dtype == np.int64 and np.array_equal(pn, g['sv_pnums'])
    assert ce.dtype == np.float32 and np.array_equal(ce, g['sv_centers'])
    prob = lio.load_prob(put('prob.npy', 'file_prob'))
    assert prob.dtype == torch.float32 and np.array_equal(prob.numpy(), g['prob'])
    sv_id, sv2point = lio.load_supervoxels(put('sv.pickle', 'file_supervoxel'))
    assert np.array_equal(sv_id, g['sv_id']) and len(sv2point) == g['sv2point'].shape[0]
    assert all(np.array_equal(a, b) for a, b in zip(sv2point, g['sv2point']))
    # and the other direction: byte-identical files for the .npy artefacts
    lio.save_sv_flag(str(tmp_path / 'w/flag1.npy'), f1)
    assert (tmp_path / 'w/flag1.npy').read_bytes() == g['file_sv_flag_1r'].tobytes()
    lio.save_sv_stats(str(tmp_path / 'w/sv_pnums.npy'), str(tmp_path / 'w/sv_centers.npy'), pn, ce)
    assert (tmp_path / 'w/sv_pnums.npy').read_bytes() == g['file_sv_pnums'].tobytes()
    assert (tmp_path / 'w/sv_centers.npy').read_bytes() == g['file_sv_centers'].tobytes()
    lio.save_prob_pred(str(tmp_path / 'w/prob.npy'), str(tmp_path / 'w/pred.npy'), prob, prob.argmax(1))
    assert (tmp_path / 'w/prob.npy').read_bytes() == g['file_prob'].tobytes()
    lio.save_supervoxels(str(tmp_path / 'w/sv.pickle'), sv_id, sv2point)
    with open(tmp_path / 'w/sv.pickle', 'rb') as f:
        a, b = pickle.load(f)
    assert np.array_equal(a, g['sv_id']) and all(np.array_equal(x, y) for x, y in zip(b, g['sv2point']))


_REF_DROPIN = r'''
import json, os, sys, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, 'tests', 'golden'))
sys.path.insert(0, os.path.join(%(root)r, 'scripts'))
import lidal_amd
lidal_amd.install_as_torchsparse()          # (default: torch's row-wise modules adopted at the first forward call)
import torchsparse                          # what a model file written against torchsparse imports
import surface_unet                         # such a file: the reference's composition and state_dict keys
from weights import state_dict_signature
from lidal_amd import io as lio
from lidal_amd.network import SPVCNN, MinkUNet
user = surface_unet.build(torchsparse)
for name, cls in (('spvcnn', SPVCNN), ('minkunet', MinkUNet)):
    ref = user[name](19)
    sig = [[k, list(s), d] for k, s, d in state_dict_signature(ref)]
    assert sig == json.load(open(os.path.join(%(root)r, 'tests', 'golden', 'state_dict_%%s.json' %% name))), name
    # train.py:151-155 under DDP (keys carry 'module.'), read back by the build's loader, strict
    path = os.path.join(%(tmp)r, name + '.pt')
    torch.save({'model_state_dict': {'module.' + k: v for k, v in ref.state_dict().items()},
                'iteration': 20000, 'ep_id': 3}, path)
    mine = cls(19)
    assert lio.load_checkpoint(path, mine) == (20000, 3)
    assert all(torch.equal(a, b) for a, b in zip(mine.state_dict().values(), ref.state_dict().values()))
print('DROPIN_OK')
'''


def test_reference_model_files_construct_over_lidal_amd(tmp_path):
    """INTEGRATION.md's claim, executed: with lidal_amd installed under the name `torchsparse`, a model file written
    against torchsparse (scripts/surface_unet.py: the reference's network/{spvcnn,minkunet}.py composition) imports and
    constructs, its state_dict is the committed checkpoint surface -- tests/golden/state_dict_*.json, written from the
    reference's own model files by make_golden.py -- and a checkpoint saved from it the way train.py does loads
    strict=True into the build's own model definitions.  (Own process: the alias stays out of this session's
    sys.modules.)"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-c', _REF_DROPIN % {'root': ROOT, 'tmp': str(tmp_path)}],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'DROPIN_OK' in r.stdout, r.stderr[-3000:]


def test_geometry_build_refuses_cpu_tensors_and_foreign_networks():
    """The coordinate tables are a GPU product like everything else: no CPU path, loud errors."""
    import pytest
    import torch
    from lidal_amd.network import Geometry, MinkUNet
    model = MinkUNet(19)
    coords = torch.zeros((10, 4), dtype=torch.int32)
    with pytest.raises(RuntimeError, match='GPU only'):
        Geometry.build(model, coords)
    with pytest.raises(TypeError, match='SPVCNN and MinkUNet'):
        Geometry.build(torch.nn.Linear(4, 4), coords)


def test_cpu_binding_is_a_no_op_when_the_topology_cannot_be_read(monkeypatch):
    """backend.bind_cpus_near(device): without a GPU (or without the sysfs entry) nothing is changed and nothing raised.
    Both cases are made here, so that on a host with a GPU the test process is not bound to its NUMA node."""
    import os
    import types
    import torch
    from lidal_amd import backend as B

    def no_gpu(index):
        raise RuntimeError('no GPU')
    no_entry = types.SimpleNamespace(pci_domain_id=0xffff, pci_bus_id=0xff, pci_device_id=0x1f)
    before = os.sched_getaffinity(0)
    for props in (no_gpu, lambda index: no_entry):
        monkeypatch.setattr(torch.cuda, 'get_device_properties', props)
        assert B.bind_cpus_near(0) is None
        assert os.sched_getaffinity(0) == before


def test_data_parallel_needs_a_process_group():
    import pytest
    import torch
    from lidal_amd.data_parallel import DataParallel
    with pytest.raises(RuntimeError, match='process group'):
        DataParallel(torch.nn.Linear(2, 2))


def test_library_holds_no_packed_f32_instructions(tmp_path):
    """lidal_amd/build.py compiles without v_pk_{mul,fma,add}_f32: on MI355X a wave executing v_mfma_f32_16x16x32_bf16
    disturbs them in waves of OTHER kernels on its SIMD (profiles/README.md, round 3), and the library runs its table
    builders and the scorer on streams beside the bf16 convolutions.  Disassembles every gfx950 code object of the
    built library (also what a variant library of scripts/build_variant.py must satisfy)."""
    import glob
    import os
    import shutil
    import subprocess
    from lidal_amd import backend as B
    objdump = '/opt/rocm/lib/llvm/bin/llvm-objdump'
    if not os.path.exists(objdump):
        import pytest
        pytest.skip('no llvm-objdump in this image')
    so = os.path.join(str(tmp_path), 'lib.so')
    shutil.copy(B.lib_path() if hasattr(B, 'lib_path') else os.path.join(os.path.dirname(B.__file__), 'liblidal_amd.so'), so)
    subprocess.run([objdump, '--offloading', so], check=True, cwd=str(tmp_path), stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    objs = glob.glob(so + '.*gfx950*')
    assert objs, 'no gfx950 code object in the library'
    mfma = packed = 0
    for o in objs:
        text = subprocess.run([objdump, '-d', o], check=True, capture_output=True, text=True).stdout
        mfma += text.count('v_mfma_f32_16x16x32_bf16')
        packed += sum(text.count(op) for op in ('v_pk_mul_f32', 'v_pk_fma_f32', 'v_pk_add_f32'))
    assert mfma > 1000, mfma            # (the disassembly really is the kernels')
    assert packed == 0, packed
