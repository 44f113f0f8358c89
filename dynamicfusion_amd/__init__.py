"""dynamicfusion_amd -- MI355X (gfx950) native DynamicFusion hot path.

Warp-field-deformed TSDF integration, surface ray-casting and the per-voxel dual-quaternion blend
(k-NN over warp nodes) as hand-written HIP kernels behind a C-ABI (include/dfusion.h), with
host-side mirrors of kfusion::cuda::TsdfVolume / kfusion::WarpField, the colour volume (ColorVolume), the depth front-end + ProjectiveICP (frontend) and the Z-slab
collectives (sharded).
"""
from . import build, capi, frontend, mesh_io, mesh_ops, sharded, synth  # noqa: F401
from .tsdf_volume import Intr, TsdfVolume, compute_dists, download_u16, upload_u16  # noqa: F401
from .warp_field import WarpField  # noqa: F401
from .color_volume import ColorVolume  # noqa: F401
from .mesh_ops import boundary_loops, closest_points, fill_holes, mesh_distance, mesh_adjacency, mesh_components, mesh_topology, ray_hits, remove_small_components, simplify_mesh, smooth_mesh, visible_points  # noqa: F401

__all__ = ["build", "capi", "frontend", "mesh_io", "mesh_ops", "sharded", "synth", "Intr", "TsdfVolume", "WarpField", "ColorVolume", "compute_dists", "upload_u16", "download_u16", "mesh_components",
           "remove_small_components", "simplify_mesh", "mesh_adjacency", "smooth_mesh", "mesh_topology", "boundary_loops", "fill_holes", "closest_points", "mesh_distance", "ray_hits", "visible_points"]
