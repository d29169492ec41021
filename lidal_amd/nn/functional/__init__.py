"""torchsparse.nn.functional surface used by the reference (network/utils.py:2):
sphash, sphashquery, spcount, spvoxelize, spdevoxelize, calc_ti_weights, spdownsample, conv3d."""
from .conv import KernelMap, build_kernel_map, conv3d
from .count import spcount
from .devoxelize import calc_ti_weights, spdevoxelize, ti_weights_and_index
from .downsample import downsample_pyramid, spdownsample, unique_sorted
from .fused import add_relu
from .hash import sphash
from .loss import combined_loss, cross_entropy, lovasz_forward, lovasz_softmax, lovasz_softmax_flat
from .query import HashTable, coords_table, sphashquery
from .voxelize import spvoxelize

__all__ = ['sphash', 'sphashquery', 'HashTable', 'coords_table', 'spcount', 'spvoxelize', 'spdevoxelize',
           'calc_ti_weights', 'ti_weights_and_index', 'spdownsample', 'downsample_pyramid', 'unique_sorted', 'conv3d',
           'add_relu', 'cross_entropy', 'lovasz_softmax', 'lovasz_softmax_flat', 'lovasz_forward', 'combined_loss',
           'KernelMap', 'build_kernel_map']
