"""Host-side mirror of kfusion::WarpField over the C-ABI (node store + k-NN + DQB on the GPU).

Mirrors /root/reference/kfusion/include/kfusion/warp_field.hpp:41-88 for the hot-path methods:
init / getNodes / KNN / warp / setWarpToLive / buildKDTree (here: the GPU brick index).
energy_data (the Opt / Ceres data term of the reference) is a conjugate-gradient solve on the GPU (dfusion_warp_solve_data_term).
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .synth import aff12, identity_dq
from .tsdf_volume import _flat, _ptr, _stream

F32 = np.float32
KNN_NEIGHBOURS = 8           # warp_field.hpp:10 (compile-time there, runtime here)


class WarpField:
    def __init__(self, k=KNN_NEIGHBOURS, device="cuda", voxel_table=True, weight_table=True, tables_on_demand=True):
        self.k = int(k)
        # fill the per-voxel tables block by block as the sweeps' launch plans first need them (DF_INDEX_TABLES_ON_DEMAND) instead of
        # all at once when the index is built; same results
        self.tables_on_demand = bool(tables_on_demand)
        self.voxel_table = bool(voxel_table)     # cache the per-voxel k-NN in HBM (k*2 B/voxel); False = re-rank per frame
        self.weight_table = bool(weight_table) and self.voxel_table   # also cache the k blend weights (k*4 B/voxel)
        self.device = torch.device(device)
        h = C.c_void_p()
        capi.check(capi.lib().dfusion_warp_create(C.byref(h)), "dfusion_warp_create")
        self.handle = h
        self.warp_to_live_ = np.eye(4, dtype=F32)      # warp_field.cpp:26
        self.M = 0
        self._index_key = None
        self._keep = []
        self._dq = None

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                capi.lib().dfusion_warp_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ---- WarpField::init(std::vector<Vec3f>) (warp_field.cpp:68-88): identity transforms, dg_w = sigma
    def init(self, vertices, sigma=3.0, transforms=None):
        pos = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
        M = pos.shape[0]
        dq = identity_dq(M) if transforms is None else np.ascontiguousarray(transforms, F32).reshape(M, 8)
        sig = np.full(M, sigma, F32) if np.isscalar(sigma) else np.ascontiguousarray(sigma, F32).reshape(M)
        self.set_nodes(torch.from_numpy(pos).to(self.device), torch.from_numpy(dq).to(self.device),
                       torch.from_numpy(sig).to(self.device))

    def set_nodes(self, pos_dev, dq_dev, sigma_dev):
        self.M = int(pos_dev.shape[0])
        self._keep = [pos_dev, dq_dev, sigma_dev]
        self._dq = dq_dev                              # the transforms the handle holds now (set_transforms / energy_data replace them)
        capi.check(capi.lib().dfusion_warp_set_nodes(self.handle, _ptr(pos_dev), _ptr(dq_dev), _ptr(sigma_dev), self.M,
                                                     _stream()), "dfusion_warp_set_nodes")
        self._index_key = None

    def extend(self, points_dev, radius, sigma=None, max_new=None, k=None):
        """Grow the field (include/dfusion.h dfusion_warp_extend): a node for the lowest-index unsupported point of every `radius` grid
        cell, dg_w = `sigma` (None: the lower median dg_w of the current nodes), at most `max_new` (None: as many as fit 65535).  The
        k-NN index, if any, is updated on the handle for the same volume geometry, so the index key stays valid.  Returns
        (n_added, n_winners).  The added nodes are kept as self.new_nodes = (pos [n,3], dq [n,8], sigma [n]) device tensors: the
        next set_transforms takes M + n_added transforms, the new nodes' following the old ones.  self._keep becomes the grown set as
        the handle now holds it (the current transforms of the old nodes, then the new ones)."""
        k = self.k if k is None else int(k)
        old_pos, old_dq, old_sigma = self._keep
        if sigma is None:
            sigma = float(torch.median(old_sigma.reshape(-1).float()).item())
        cap = max(0, 65535 - self.M) if max_new is None else int(max_new)
        pts = points_dev.reshape(-1, 3)
        n = int(pts.shape[0])
        m = max(0, min(cap, n))
        new_pos = torch.empty((m, 3), dtype=torch.float32, device=self.device)
        new_dq = torch.empty((m, 8), dtype=torch.float32, device=self.device)
        new_sigma = torch.empty(m, dtype=torch.float32, device=self.device)
        added, winners = C.c_int(0), C.c_int(0)
        rc = (capi.lib().dfusion_warp_extend(self.handle, k, _flat(pts) if n else None, n, float(radius), float(sigma), cap,
                                                  _ptr(new_pos) if m else None, _ptr(new_dq) if m else None, _ptr(new_sigma) if m else None,
                                                  C.byref(added), C.byref(winners), _stream()))
        a = added.value                                # (also set when the nodes went in and a later step failed: the handle holds them)
        self.new_nodes = (new_pos[:a], new_dq[:a], new_sigma[:a])
        if a:
            self.M += a
            cur = self._dq if self._dq is not None else old_dq
            self._keep = [torch.cat([old_pos.reshape(-1, 3), new_pos[:a]]), torch.cat([cur.reshape(-1, 8), new_dq[:a]]),
                          torch.cat([old_sigma.reshape(-1), new_sigma[:a]])]
            self._dq = self._keep[1]
        if rc != 0:
            self._index_key = None                     # (the index update did not complete)
        capi.check(rc, "dfusion_warp_extend")
        return a, winners.value

    def set_transforms(self, dq_dev):
        """What the warp optimiser writes back every frame (CombinedSolver.h:189-197)."""
        capi.check(capi.lib().dfusion_warp_set_transforms(self.handle, _ptr(dq_dev), _stream()),
                   "dfusion_warp_set_transforms")
        self._dq = dq_dev

    def setWarpToLive(self, pose):     # warp_field.cpp:302-305
        self.warp_to_live_ = np.asarray(pose, F32).reshape(4, 4).copy()

    # ---- buildKDTree (warp_field.cpp:275-282) -> exact k-NN brick index for one volume geometry
    def ensure_index(self, volume, k):
        key = (volume.getDims(), tuple(volume.getVoxelSize().tolist()), volume.getPose().tobytes(),
               (volume.z_own0, volume.z_own_n), int(k))
        if self._index_key is not None and self._index_key[:4] == key[:4] and (
                self._index_key[4] == k or (not self.voxel_table and self._index_key[4] >= k)):
            return
        capi.check(capi.lib().dfusion_warp_build_index(self.handle, volume.c_volume(), volume.c_slab(),
                                                       capi.floats(aff12(volume.getPose())), int(k),
                                                       (capi.DF_INDEX_VOXEL_TABLE if self.voxel_table else 0) |
                                                       (capi.DF_INDEX_WEIGHT_TABLE if self.weight_table else 0) |
                                                       (capi.DF_INDEX_TABLES_ON_DEMAND if self.tables_on_demand else 0), _stream()),
                   "dfusion_warp_build_index")
        self._index_key = key

    # ---- WarpField::KNN (warp_field.cpp:247-251), batched
    def KNN(self, queries_dev, k=None):
        k = self.k if k is None else k
        n = int(queries_dev.shape[0])
        idx = torch.empty((n, k), dtype=torch.int32, device=self.device)
        d2 = torch.empty((n, k), dtype=torch.float32, device=self.device)
        capi.check(capi.lib().dfusion_knn(self.handle, k, _flat(queries_dev), n, _ptr(idx), _ptr(d2), _stream()),
                   "dfusion_knn")
        return idx, d2

    # ---- WarpField::warp (warp_field.cpp:180-195), in place on device [N,3] tensors
    def warp(self, points_dev, normals_dev=None, k=None):
        k = self.k if k is None else k
        n = int(points_dev.shape[0])
        capi.check(capi.lib().dfusion_warp_points(self.handle, k, _flat(points_dev),
                                                  _flat(normals_dev) if normals_dev is not None else None, n,
                                                  capi.floats(aff12(self.warp_to_live_)), _stream()),
                   "dfusion_warp_points")

    def debug_counters(self, swept_dev=None):
        """Measurement hook (include/dfusion.h dfusion_warp_debug_counters): while set (device int64[1]), every warped integrate through
        THIS field adds the voxels its launch plan keeps; None switches it off."""
        capi.check(capi.lib().dfusion_warp_debug_counters(self.handle, _ptr(swept_dev) if swept_dev is not None else None),
                   "dfusion_warp_debug_counters")

    def alive_blocks_per_layer(self, volume, layers_dev):
        """layers_dev (device int64 [Z / 8]) += the 8x8x8 blocks the last sweep's verdict pass kept, per 8-plane layer, for the layers
        inside `volume`'s OWN planes (Z-slab re-balancing; include/dfusion.h dfusion_warp_alive_blocks)."""
        capi.check(capi.lib().dfusion_warp_alive_blocks(self.handle, int(volume.z_own0), int(volume.z_own_n), _ptr(layers_dev),
                                                        int(layers_dev.numel()), _stream()), "dfusion_warp_alive_blocks")
        return layers_dev

    def coded_blocks_per_layer(self, volume, layers_dev):
        """The kept blocks among those that had 4-bit neighbour codes (include/dfusion.h dfusion_warp_coded_blocks)."""
        capi.check(capi.lib().dfusion_warp_coded_blocks(self.handle, int(volume.z_own0), int(volume.z_own_n), _ptr(layers_dev),
                                                        int(layers_dev.numel()), _stream()), "dfusion_warp_coded_blocks")

    def set_point_tiling(self, image_cols):
        """Locality hint (include/dfusion.h dfusion_warp_set_point_tiling): point queries are row-major images `image_cols` wide and are
        processed in 8x8 pixel tiles per wave; 0 = off.  Results do not change."""
        capi.check(capi.lib().dfusion_warp_set_point_tiling(self.handle, int(image_cols)), "dfusion_warp_set_point_tiling")

    # ---- WarpField::energy_data (warp_field.cpp:117-163) / WarpFieldOptimiser::optimiseWarpData: the warp solves, on the GPU
    def _solve(self, fn, canonical_dev, live_dev, k, iters, damping, reg=None, robust=None, normals=(), return_weights=False):
        """What the solves below share.  Calls the C function `fn`(handle, k, canonical, live, *normals, n, iters, *damping, *reg, *robust,
        dq, energy[, point_weights, edge_weights], stream): `normals` is () where fn takes none, else (tensor or None,); `reg` is None or
        (reg_neighbours, reg_lambda), with which the energy has 4 entries instead of 2; `robust` is None or (rounds, tukey_c, huber_delta),
        with which fn has the two weight outputs.  Returns (dq, energy) and, with return_weights, (point_weights, edge_weights or None
        without edges); the transforms the handle holds are dq from here on."""
        k = self.k if k is None else k
        n = int(canonical_dev.shape[0])
        for nrm in normals:
            if nrm is not None and int(nrm.numel()) != 3 * n:
                raise ValueError("one normal per point expected (%d points, normals of shape %s)" % (n, tuple(nrm.shape)))
        reg = () if reg is None else (int(reg[0]), float(reg[1]))
        dq = torch.empty((self.M, 8), dtype=torch.float32, device=self.device)
        en = torch.zeros(4 if reg else 2, dtype=torch.float32, device=self.device)
        pw = ew = None
        if return_weights:
            pw = torch.empty(n, dtype=torch.float32, device=self.device)
            if reg and reg[0] > 0 and reg[1] != 0.0:
                ew = torch.empty((self.M, reg[0]), dtype=torch.float32, device=self.device)
        outs = [dq, en] + ([] if robust is None else [pw, ew])
        robust = () if robust is None else (int(robust[0]), float(robust[1]), float(robust[2]))
        capi.check(getattr(capi.lib(), fn)(self.handle, k, _flat(canonical_dev), _flat(live_dev), *[None if t is None else _flat(t) for t in normals], n,
                                           int(iters), *[float(d) for d in damping], *reg, *robust, *[None if t is None else _ptr(t) for t in outs],
                                           _stream()), fn)
        self._dq = dq
        return (dq, en, pw, ew) if return_weights else (dq, en)

    def energy_data(self, canonical_dev, live_dev, iters=100, lam=0.0, k=None):
        """Least-squares update of the node translations so that canonical + sum_i w_i T_i meets live (device [N,3] tensors).
        Returns (dq [M,8] device tensor of the updated transforms, energy [before, after] device tensor)."""
        return self._solve("dfusion_warp_solve_data_term", canonical_dev, live_dev, k, iters, (lam,))

    def solve(self, canonical_dev, live_dev, iters=100, lam=0.0, reg_neighbours=0, reg_lambda=0.0, k=None):
        """energy_data with DynamicFusion's regularisation term over the node graph (include/dfusion.h dfusion_warp_solve): every node
        is tied to its `reg_neighbours` nearest other nodes with weight `reg_lambda`, so that nodes few or no points constrain follow
        their neighbours.  reg_neighbours = 0 or reg_lambda = 0: energy_data's result.  Returns (dq [M,8] device tensor, energy device
        tensor [E_data before, E_data after, E_reg before, E_reg after])."""
        return self._solve("dfusion_warp_solve", canonical_dev, live_dev, k, iters, (lam,), (reg_neighbours, reg_lambda))

    def solve_robust(self, canonical_dev, live_dev, iters=100, lam=0.0, reg_neighbours=0, reg_lambda=0.0, rounds=3, tukey_c=0.0,
                     huber_delta=0.0, k=None, return_weights=False):
        """solve with DynamicFusion's robust penalties by iteratively re-weighted least squares (include/dfusion.h
        dfusion_warp_solve_robust): `rounds` solves, each weighting every point with the Tukey weight of its residual (threshold
        `tukey_c`, 0 = off) and every graph edge with the Huber weight of its difference (threshold `huber_delta`, 0 = off) at the
        transforms the round starts from.  Returns (dq [M,8] device tensor, energy device tensor [E_data before, E_data after, E_reg
        before, E_reg after]) and, with return_weights, (point_weights [N], edge_weights [M, reg_neighbours] or None without edges): the
        last round's weights -- 0 marks a point the solve ignored."""
        return self._solve("dfusion_warp_solve_robust", canonical_dev, live_dev, k, iters, (lam,), (reg_neighbours, reg_lambda),
                           (rounds, tukey_c, huber_delta), return_weights=return_weights)

    def solve_plane(self, canonical_dev, live_dev, normals_dev, iters=100, lam=0.0, reg_neighbours=0, reg_lambda=0.0, rounds=1, tukey_c=0.0,
                    huber_delta=0.0, k=None, return_weights=False):
        """solve_robust with the point-to-plane data term (include/dfusion.h dfusion_warp_solve_plane): the residual of every point is
        taken along its normal (`normals_dev`, device [N,3], in the frame of the points, used as given), so that a live point that slid
        along the surface -- what projective association leaves -- does not pull on the nodes.  A point with a NaN or infinite normal
        is skipped.  Returns what solve_robust returns; the data energies are those of the projected residual."""
        return self._solve("dfusion_warp_solve_plane", canonical_dev, live_dev, k, iters, (lam,), (reg_neighbours, reg_lambda),
                           (rounds, tukey_c, huber_delta), (normals_dev,), return_weights)

    def solve_rigid(self, canonical_dev, live_dev, normals_dev=None, iters=100, lam=0.0, lam_rot=0.0, reg_neighbours=0, reg_lambda=0.0, rounds=1,
                    tukey_c=0.0, huber_delta=0.0, k=None, return_weights=False):
        """The solve with the node rotations as unknowns too (include/dfusion.h dfusion_warp_solve_rigid): `rounds` Gauss-Newton rounds
        against the DQB warp that warp() and the warped integrate apply, six unknowns a node, `lam_rot` damping the rotations as `lam`
        damps the translations.  `canonical_dev` and `normals_dev` are the UNWARPED model points and normals (the solve warps them
        itself); normals_dev None: the point-to-point data term, otherwise the residual along the warped normal.  Returns what
        solve_robust returns; the data energy `after` is that of the warp at the transforms written, not of the linearisation."""
        return self._solve("dfusion_warp_solve_rigid", canonical_dev, live_dev, k, iters, (lam, lam_rot), (reg_neighbours, reg_lambda),
                           (rounds, tukey_c, huber_delta), (normals_dev,), return_weights)

    def node_graph(self, kg):
        """The graph solve() regularises over: (nbr int32 [M, kg], alpha float32 [M, kg]) device tensors -- node i's kg nearest other
        nodes and the edge weights max(dg_w_i, dg_w_j)."""
        kg = int(kg)
        nbr = torch.empty((self.M, max(kg, 0)), dtype=torch.int32, device=self.device)
        alpha = torch.empty((self.M, max(kg, 0)), dtype=torch.float32, device=self.device)
        capi.check(capi.lib().dfusion_warp_node_graph(self.handle, kg, _ptr(nbr), _ptr(alpha), _stream()), "dfusion_warp_node_graph")
        return nbr, alpha

    def set_graph_hierarchy(self, levels, radius, beta=4.0):
        """Regularise over DynamicFusion's hierarchy of nodes instead of the flat graph (include/dfusion.h
        dfusion_warp_set_graph_hierarchy): level l keeps one node per cell of edge radius * beta^(l-1) of the level below, and a node's
        edges go to its nearest nodes one level up, so a correction crosses a long unobserved stretch in a few steps.  levels = 0
        switches it off.  The setting stays on the field; extend and set_nodes only drop the graph built from it."""
        capi.check(capi.lib().dfusion_warp_set_graph_hierarchy(self.handle, int(levels), float(radius), float(beta)),
                   "dfusion_warp_set_graph_hierarchy")

    def graph_levels(self, kg):
        """The levels behind node_graph(kg): (top int32 [M] the highest level of every node, sizes int32 [9] |S_0| .. |S_8|, effective
        int32 [1] the depth in use; 0: the flat graph) device tensors."""
        top = torch.empty(self.M, dtype=torch.int32, device=self.device)
        sizes = torch.empty(9, dtype=torch.int32, device=self.device)
        effective = torch.empty(1, dtype=torch.int32, device=self.device)
        capi.check(capi.lib().dfusion_warp_graph_levels(self.handle, int(kg), _ptr(top), _ptr(sizes), _ptr(effective), _stream()),
                   "dfusion_warp_graph_levels")
        return top, sizes, effective

    def set_preconditioner(self, mode):
        """The preconditioner of solve_rigid's conjugate gradients (include/dfusion.h dfusion_warp_set_preconditioner): 0 none (the
        default), 1 the 6x6 diagonal block of every node (its rotation and translation together), rebuilt and factored every round.  The
        setting stays on the field through extend, set_nodes and set_transforms; solve, solve_robust and solve_plane do not read it."""
        capi.check(capi.lib().dfusion_warp_set_preconditioner(self.handle, int(mode)), "dfusion_warp_set_preconditioner")

    @property
    def preconditioner(self):
        mode = C.c_int(-1)
        capi.check(capi.lib().dfusion_warp_preconditioner(self.handle, C.byref(mode)), "dfusion_warp_preconditioner")
        return mode.value
