"""In-tree build of the gfx950 HIP library (libdfusion_hip.so) with hipcc.

The .so is git-ignored but travels to the GPU box with the gpurun snapshot, so a box without
the sources' mtimes changing never rebuilds.  hipcc cross-compiles without a GPU.
"""
import os
import re
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(PKG_DIR, "libdfusion_hip.so")

SOURCES = ["dfusion_volume.hip", "dfusion_warp.hip", "dfusion_warp_nodes.hip", "dfusion_warp_points.hip", "dfusion_warp_index.hip",
           "dfusion_raycast.hip", "dfusion_frontend.hip", "dfusion_solver.hip", "dfusion_selftest.hip", "dfusion_warp_extend.hip", "dfusion_mesh.hip", "dfusion_associate.hip", "dfusion_color.hip", "dfusion_render.hip",
           "dfusion_warp_graph.hip", "dfusion_mesh_components.hip", "dfusion_mesh_simplify.hip", "dfusion_mesh_smooth.hip", "dfusion_mesh_holes.hip", "dfusion_mesh_bvh.hip", "dfusion_mesh_rays.hip"]
HEADERS = ["dfusion_device.h", "dfusion_internal.h", "dfusion_nanoflann.h", "dfusion_pyramid.h", "dfusion_warp_topk.h", "dfusion_warp_sweep.h",
           "dfusion_warp_blocks.h", "dfusion_warp_pipe.h", "dfusion_plan_halves.h", "dfusion_warp_decide.h", "dfusion_mesh_cc.h", "dfusion_mesh_kit.h", "dfusion_mesh_uses.h", "dfusion_mesh_bvh.h", os.path.join(REPO_DIR, "include", "dfusion.h")]

# -ffp-contract=off: fused multiply-adds only where the reference writes __fmaf_rn (explicit fmaf);
# that is what makes the kernels bit-comparable with the IEEE CPU oracle.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-fno-fast-math", "-Wno-unused-result"]


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the dynamicfusion_amd HIP library cannot be built")


def _stale():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [h if os.path.isabs(h) else os.path.join(CSRC, h) for h in HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def _csrc_includes(name, seen):
    """`name` and every csrc header it includes (transitively), each once, in include order."""
    if name in seen:
        return seen
    seen.append(name)
    for inc in re.findall(r'^#include "([^"]+)"', open(os.path.join(CSRC, name)).read(), re.M):
        if os.path.exists(os.path.join(CSRC, inc)):
            _csrc_includes(inc, seen)
    return seen


def kernel_source_sha(kernel):
    """sha256 over the sources a kernel (by name) is built from: the .hip that emits it and exactly the csrc headers that .hip includes.
    Stamps profiles/pmc_latest.json (tools/pmc_summary.py); bench.py drops counters whose stamp is not the tree's."""
    import hashlib
    k = kernel.replace("void ", "")
    f = ("dfusion_warp_nodes.hip" if k.startswith(("df_pack", "df_node"))
         else "dfusion_warp_points.hip" if k.startswith("df_points")
         else "dfusion_warp_index.hip" if k.startswith(("df_brick", "df_scan", "df_grow"))
         else "dfusion_warp.hip" if k.startswith(("df_warp", "df_sweep", "df_block", "df_blocks", "df_sub", "df_dists_max", "df_alive"))
         else "dfusion_raycast.hip" if k.startswith(("df_raycast", "df_extract"))
         else "dfusion_solver.hip" if k.startswith("df_sv")
         else "dfusion_warp_graph.hip" if k.startswith("df_hg")
         else "dfusion_mesh_components.hip" if k.startswith("df_mcc_")
         else "dfusion_mesh_simplify.hip" if k.startswith("df_msp_")
         else "dfusion_mesh_smooth.hip" if k.startswith("df_msm_")
         else "dfusion_mesh_holes.hip" if k.startswith("df_mhl_")
         else "dfusion_mesh_bvh.hip" if k.startswith("df_mbv_")
         else "dfusion_mesh_rays.hip" if k.startswith("df_mry_")
         else "dfusion_mesh.hip" if k.startswith("df_mesh")
         else "dfusion_associate.hip" if k.startswith("df_assoc")
         else "dfusion_color.hip" if k.startswith("df_color")
         else "dfusion_render.hip" if k.startswith("df_render")
         else "dfusion_volume.hip")
    h = hashlib.sha256()
    for name in _csrc_includes(f, []):
        h.update(open(os.path.join(CSRC, name), "rb").read())
    return h.hexdigest()


def build_library(force=False, verbose=False):
    """Compile every HIP source for gfx950 into dynamicfusion_amd/libdfusion_hip.so."""
    if not force and not _stale():
        return LIB_PATH
    cmd = [_hipcc()] + HIPCC_FLAGS + ["-I", os.path.join(REPO_DIR, "include"), "-I", CSRC]
    cmd += [os.path.join(CSRC, s) for s in SOURCES] + ["-o", LIB_PATH + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    os.replace(LIB_PATH + ".tmp", LIB_PATH)
    return LIB_PATH


HOST_DIR = os.path.join(PKG_DIR, "host")
HOST_LIB = os.path.join(HOST_DIR, "libkfusion_hip.so")
HOST_APP = os.path.join(HOST_DIR, "headless_frame")
HOST_KINFU_APP = os.path.join(HOST_DIR, "kinfu_headless")
HOST_WARP_TESTS = os.path.join(HOST_DIR, "warp_tests")
HOST_DEMO_CALLS = os.path.join(HOST_DIR, "demo_calls")
HOST_WARP_SOLVE = os.path.join(HOST_DIR, "warp_solve")
HOST_ASSOCIATE = os.path.join(HOST_DIR, "associate")
HOST_COLOR_FRAME = os.path.join(HOST_DIR, "color_frame")
HOST_RENDER_MESH = os.path.join(HOST_DIR, "render_mesh")
HOST_SIMPLIFY_MESH = os.path.join(HOST_DIR, "simplify_mesh")
HOST_SMOOTH_MESH = os.path.join(HOST_DIR, "smooth_mesh")
HOST_FILL_HOLES = os.path.join(HOST_DIR, "fill_holes")
HOST_MESH_DISTANCE = os.path.join(HOST_DIR, "mesh_distance")
HOST_MESH_RAYS = os.path.join(HOST_DIR, "mesh_rays")
HOST_ZSLAB_LIB = os.path.join(HOST_DIR, "libkfusion_zslab.so")       # kfusion::cuda::ZSlabComm: the RCCL side of the Z-slab sharding
HOST_ZSLAB_APP = os.path.join(HOST_DIR, "zslab_frame")
# the apps over libkfusion_hip.so, in build order: host/<name> from host/apps/<name>.cpp (zslab_frame also links libkfusion_zslab.so and rccl)
HOST_APPS = [HOST_APP, HOST_KINFU_APP, HOST_WARP_TESTS, HOST_DEMO_CALLS, HOST_WARP_SOLVE, HOST_ASSOCIATE, HOST_COLOR_FRAME, HOST_RENDER_MESH, HOST_SIMPLIFY_MESH, HOST_SMOOTH_MESH, HOST_FILL_HOLES, HOST_MESH_DISTANCE, HOST_MESH_RAYS, HOST_ZSLAB_APP]


def build_host(force=False, verbose=False):
    """C++ host mirror (kfusion::cuda::TsdfVolume / WarpField over the C-ABI) + the headless harness, with g++."""
    build_library(force=False)
    src = os.path.join(HOST_DIR, "src", "kfusion_hip.cpp")
    zsrc = os.path.join(HOST_DIR, "src", "zslab_rccl.cpp")
    apps = [(os.path.join(HOST_DIR, "apps", os.path.basename(out) + ".cpp"), out) for out in HOST_APPS]
    deps = [src, zsrc, LIB_PATH] + [a for a, _ in apps] + [os.path.join(r, f) for r, _, fs in os.walk(os.path.join(HOST_DIR, "include")) for f in fs]
    outs = [HOST_LIB, HOST_ZSLAB_LIB] + [o for _, o in apps]
    if not force and all(os.path.exists(f) for f in outs) and min(os.path.getmtime(f) for f in outs) >= max(os.path.getmtime(d) for d in deps):
        return HOST_LIB, HOST_APP
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    common = ["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(HOST_DIR, "include"),
              "-I", os.path.join(REPO_DIR, "include"), "-I", os.path.join(rocm, "include")]
    link = ["-L", PKG_DIR, "-ldfusion_hip", "-L", os.path.join(rocm, "lib"), "-lamdhip64"]
    rpaths = ["-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/.."]
    cmds = [common + ["-fPIC", "-shared", src, "-o", HOST_LIB] + link + ["-Wl,-rpath,$ORIGIN/.."]]
    for app, out in apps:
        if out == HOST_ZSLAB_APP:
            cmds.append(common + ["-fPIC", "-shared", zsrc, "-o", HOST_ZSLAB_LIB, "-L", HOST_DIR, "-lkfusion_hip"] + link + ["-lrccl"] + rpaths)
            cmds.append(common + [app, "-o", out, "-L", HOST_DIR, "-lkfusion_zslab", "-lkfusion_hip"] + link + ["-lrccl"] + rpaths)
        else:
            cmds.append(common + [app, "-o", out, "-L", HOST_DIR, "-lkfusion_hip"] + link + rpaths)
    for c in cmds:
        if verbose:
            print(" ".join(c))
        subprocess.check_call(c)
    return HOST_LIB, HOST_APP


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
    print(build_host(force=True, verbose=True))
