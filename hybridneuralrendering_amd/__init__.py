"""hybridneuralrendering_amd: MI355X-native hot path of CVMI-Lab/HybridNeuralRendering.

voxel k-NN neural-point query -> point/image feature gather + aggregation MLP -> alpha composite,
as hand-written gfx950 HIP kernels behind a C ABI (include/hnr.h, libhnr_hip.so) with a host-side
mirror of the reference's module surface.  See DESIGN.md and INTEGRATION.md.
"""
from . import scenes  # noqa: F401
from ._lib import HnrError  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # heavier modules are imported lazily so that `import hybridneuralrendering_amd` works without a GPU
    if name in ("lighting_fast_querier", "VoxelGrid", "march_query", "compact_rays", "tmid_table"):
        from . import querier
        return getattr(querier, name)
    if name in ("MVSNet", "depth_views"):
        from . import mvs_depth
        return getattr(mvs_depth, name)
    if name in ("AlphaMasks", "alpha_masking", "visual_hull_select", "point_occlusion", "init_cloud_from_mvs_depth"):
        from . import cloud_init
        return getattr(cloud_init, name)
    if name == "RAFT":
        from . import flow
        return flow.RAFT
    if name == "LPIPS":
        from . import perceptual
        return perceptual.LPIPS
    if name in ("content_aware_weights", "weights_from_scores"):
        from . import frame_weights
        return getattr(frame_weights, name)
    if name in ("DeviceAdam", "ShellOptimizers"):
        from . import optim
        return getattr(optim, name)
    raise AttributeError(name)
