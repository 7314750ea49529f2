"""Host-side mirror of the reference's assembler interface for the hot path.

``Assembler`` plays the role of the slice of ``FracturePhaseFieldProblem<dim>`` that
owns ``assemble_system(bool residual_only)`` / ``assemble_nl_residual()``
(cracks.cc:2129-2512): same member names (``solution``, ``old_solution``,
``old_old_solution``, ``system_pde_matrix``, ``system_pde_residual``,
``system_total_residual``), same call shapes, same error behaviour (exceptions where the
reference throws / aborts).  All arithmetic happens in the HIP library behind the C ABI
(``include/pfm_assemble.h``); PyTorch only provides device memory, streams and — in
``cracks_amd.halo`` — ``torch.distributed`` (RCCL).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import capi
from .capi import PfmError, PfmParams


def node_flags_from_dof_flags(layout, update_flag: np.ndarray, hanging_flag: Optional[np.ndarray] = None) -> np.ndarray:
    """One byte per node, bit c = dof (node, c) carries a homogeneous line of
    ``constraints_update`` that is not a hanging-node line (those travel in the mesh
    description)."""
    n = np.arange(layout.n_nodes)
    flags = np.zeros(layout.n_nodes, np.uint8)
    for c in range(layout.nc):
        d = layout.dof(n, c)
        f = update_flag[d].astype(bool)
        if hanging_flag is not None:
            f &= ~hanging_flag[d].astype(bool)
        flags |= (f.astype(np.uint8) << c).astype(np.uint8)
    return flags


class Context:
    """RAII wrapper of ``pfm_ctx``."""

    def __init__(self, mesh, blocked: bool, device: int = 0, n_owned_nodes: Optional[int] = None,
                 cell_lambda: Optional[np.ndarray] = None, cell_mu: Optional[np.ndarray] = None):
        self.lib = capi.load()
        self.dim = mesh.dim
        self.blocked = bool(blocked)
        self.n_nodes = mesh.n_nodes
        self.n_cells = mesh.n_cells
        self.n_owned =mesh.n_nodes if n_owned_nodes is None else int(n_owned_nodes)
        self.n_blocks = 4 if blocked else 1
        d = capi.PfmMeshDesc()
        d.dim = mesh.dim
        d.layout = capi.LAYOUT_BLOCKED if blocked else capi.LAYOUT_INTERLEAVED
        d.n_nodes = mesh.n_nodes
        d.n_owned_nodes = self.n_owned
        d.n_cells = mesh.n_cells
        keep = []

        def arr(a, dt):
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data

        d.cell_nodes = arr(mesh.cells, np.int32)
        d.coords = arr(mesh.coords, np.float64)
        if cell_lambda is not None:
            d.cell_lambda = arr(cell_lambda, np.float64)
            d.cell_mu = arr(cell_mu, np.float64)
        d.n_hanging = int(mesh.hn_nodes.size)
        if d.n_hanging:
            d.hn_nodes = arr(mesh.hn_nodes, np.int32)
            d.hn_ptr = arr(mesh.hn_ptr, np.int64)
            d.hn_parents = arr(mesh.hn_parents, np.int32)
            d.hn_weights = arr(mesh.hn_weights, np.float64)
        if getattr(mesh, "box_shape", None):
            for k, v in enumerate(mesh.box_shape):
                d.box_cells[k] = int(v)
        self._h = C.c_void_p()
        import time as _time
        _t0 = _time.perf_counter()
        rc = self.lib.pfm_ctx_create(C.byref(self._h), C.byref(d), int(device))
        self.create_seconds = _time.perf_counter() - _t0  # pfm_ctx_create alone (synchronous): the cost after every refine_mesh
        if rc != capi.PFM_OK:
            msg = self.lib.pfm_last_error(self._h).decode() if self._h else ""
            if self._h:
                self.lib.pfm_ctx_destroy(self._h)
                self._h = C.c_void_p()
            raise PfmError(rc, "pfm_ctx_create", msg)
        self.n_owned_dofs = self.n_owned * (self.dim + 1)
        self.split_model = capi.SPLIT_REFERENCE  # what set_split_model last set (pfm_set_split_model)
        self.split_route = capi.SPLIT_ROUTE_GENERAL  # what set_split_route last set (pfm_set_split_route)
        self.hanging_mode = capi.HANGING_MODE_DEFAULT  # what set_hanging_mode last set (pfm_set_hanging_mode)

    # -- helpers ---------------------------------------------------------------------
    def _check(self, rc: int, where: str):
        if rc != capi.PFM_OK:
            raise PfmError(rc, where, self.lib.pfm_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None):
            self.lib.pfm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- C ABI -----------------------------------------------------------------------
    def set_stream(self, stream_handle: int):
        self._check(self.lib.pfm_ctx_set_stream(self._h, C.c_void_p(stream_handle)), "pfm_ctx_set_stream")

    def set_split_model(self, model: int):
        """0: the reference's closed form (2-D; a 3-D split assembly is refused), 1: the spectral split of 3-D contexts,
        3: their volumetric-deviatoric split (capi.SPLIT_*; both laws in cracks_amd/split3d.py; 2 is unassigned).  Before
        set_params; a living context may change between 1 and 3 at any time."""
        self._check(self.lib.pfm_set_split_model(self._h, int(model)), "pfm_set_split_model")
        self.split_model = int(model)

    def set_split_route(self, route: int):
        """Which kernels take the residual-only assembly of a 3-D context under a split law (capi.SPLIT_ROUTE_*): 0 the
        general family over all cells (default), 1 the row-owner residual kernel of the box, the sub-box or the level lattices
        with the law at its q-points under model 3 (no effect on model 1), 3 the same kernel under model 3 and under model 1,
        the spectral law.  5 (= 1 | 4) and 7 (= 3 | 4): the same residual-only calls, and under model 3 the full assembly of a
        box or a partitioned sub-box on the row-owner kernels as well (k_cart_split3_jac; not on the level lattices of an overlay,
        not under model 1); 4 and 6 are refused.  13 (= 5 | 8) and 15 (= 7 | 8): the same, and the level lattices of a 3-D overlay take
        that full assembly too (level form of k_cart_split3_jac; regular rows then have residual_pde of the full and of the
        residual-only call bit for bit equal); every other value with bit 8 is refused.  21 (= 5 | 16) and 23 (= 7 | 16): routes 5 and 7 with the full assembly of a
        box or sub-box evaluating the law only where it differs from the unsplit one (k_cart_split3_mark, the unsplit k_cart_uu3
        and k_cart_phi4 over the whole box, then the sparse form of k_cart_split3_jac over the rows at compressed cells: those rows
        are route 5's bytes, the others the unsplit kernels'); every other value with bit 16 is refused.  61 (= 13 | 16 | 32) and
        63 (= 15 | 16 | 32): routes 13 and 15 with that sparse full assembly on every level lattice of a 3-D overlay (the level forms
        of k_cart_split3_mark and of the sparse k_cart_split3_jac around the unsplit level kernels: the regular rows at compressed
        cells are route 13's bytes, the other regular rows the unsplit level kernels', the general family as under 13); on a
        box they are 21 and 23; every other value with bit 32 is refused.  At any time on a living context; routes 0, 1 and 3 have no effect on full
        assemblies."""
        self._check(self.lib.pfm_set_split_route(self._h, int(route)), "pfm_set_split_route")
        self.split_route = int(route)

    def split_route_info(self):
        """(route set, whether a residual-only assembly with the current parameters, model and forced path would run the
        split law on the row-owner kernels): pfm_ctx_split_route."""
        a, b = C.c_int32(-1), C.c_int32(-1)
        self._check(self.lib.pfm_ctx_split_route(self._h, C.byref(a), C.byref(b)), "pfm_ctx_split_route")
        return int(a.value), int(b.value)

    def split_route_plan(self):
        """(route set, whether the residual-only assembly would run its law on the row-owner kernels, whether the full
        assembly would, cells with a compressed q-point counted by the last full assembly on those kernels or -1):
        pfm_ctx_split_route_info, answered from the assembly plan.  split_route_info() keeps its two answers."""
        out = (C.c_int64 * 4)(-1, -1, -1, -1)
        self._check(self.lib.pfm_ctx_split_route_info(self._h, out), "pfm_ctx_split_route_info")
        return tuple(int(x) for x in out)

    def split_sparse_info(self):
        """(whether a full assembly with the current parameters, model, route and forced path would run sparse, nodes whose
        rows the sparse form of k_cart_split3_jac recomputed in the last full assembly or -1 if that one did not run sparse,
        tile-chunks flagged in it or -1, tile-chunks of the grid): pfm_ctx_split_sparse_info.  On a 3-D overlay under routes 61 /
        63 the rows, flags and tile-chunks are summed over the level lattices."""
        out = (C.c_int64 * 4)(-1, -1, -1, -1)
        self._check(self.lib.pfm_ctx_split_sparse_info(self._h, out), "pfm_ctx_split_sparse_info")
        return tuple(int(x) for x in out)

    def set_hanging_mode(self, mode: int):
        """How the cells at hanging vertices reach the outputs (capi.HANGING_MODE_*): 0 as ever (3-D unsplit and model 3:
        scratch + ordered gather; 3-D model 1 and 2-D: atomic adds), 1 scratch + ordered gather in both dimensions and under
        every law (bitwise reproducible), 2 the atomic class everywhere.  At any time on a living context."""
        self._check(self.lib.pfm_set_hanging_mode(self._h, int(mode)), "pfm_set_hanging_mode")
        self.hanging_mode = int(mode)

    def hanging_info(self):
        """(mode set, [cells at hanging vertices, the next assembly gathers them, rows of the gather tables, device bytes of
        tables and scratch, the next assembly issues floating-point atomic adds]): pfm_ctx_hanging_info."""
        m, out = C.c_int32(-1), (C.c_int64 * 5)()
        self._check(self.lib.pfm_ctx_hanging_info(self._h, C.byref(m), out), "pfm_ctx_hanging_info")
        return int(m.value), [int(x) for x in out]

    def set_params(self, prm):
        p = prm if isinstance(prm, PfmParams) else PfmParams.from_any(prm)
        self._check(self.lib.pfm_set_params(self._h, C.byref(p)), "pfm_set_params")

    def set_constraints(self, node_flags: np.ndarray):
        f = np.ascontiguousarray(node_flags, np.uint8)
        assert f.size == self.n_nodes
        self._check(self.lib.pfm_set_constraints(self._h, capi.np_ptr(f, np.uint8)), "pfm_set_constraints")

    def pattern_size(self, block: int):
        r, z = C.c_int64(), C.c_int64()
        self._check(self.lib.pfm_pattern_size(self._h, block, C.byref(r), C.byref(z)), "pfm_pattern_size")
        return r.value, z.value

    def pattern(self, block: int):
        rows, nnz = self.pattern_size(block)
        rowptr = np.zeros(rows + 1, np.int64)
        colind = np.zeros(nnz, np.int32)
        self._check(self.lib.pfm_pattern_get(self._h, block, capi.np_ptr(rowptr, np.int64),
                                             capi.np_ptr(colind, np.int32)), "pfm_pattern_get")
        return rowptr, colind

    def pattern_bind(self, block: int, rowptr: np.ndarray, colind: np.ndarray):
        """``pfm_pattern_bind``: adopt the host's CSR arrays of one block (int64 or int32 row pointers)."""
        ci = np.ascontiguousarray(colind, np.int32)
        if np.asarray(rowptr).dtype == np.int32:
            rp = np.ascontiguousarray(rowptr, np.int32)
            rc = self.lib.pfm_pattern_bind_i32(self._h, block, capi.np_ptr(rp, np.int32), capi.np_ptr(ci, np.int32))
        else:
            rp = np.ascontiguousarray(rowptr, np.int64)
            rc = self.lib.pfm_pattern_bind(self._h, block, capi.np_ptr(rp, np.int64), capi.np_ptr(ci, np.int32))
        self._check(rc, "pfm_pattern_bind")

    def halo_exchange(self, comm_handle: int, peer_ranks):
        """``pfm_halo_exchange``: pack -> RCCL send/recv -> unpack inside the library (context's stream)."""
        pr = np.ascontiguousarray(peer_ranks, np.int32)
        self._check(self.lib.pfm_halo_exchange(self._h, C.c_void_p(comm_handle),
                                               capi.np_ptr(pr, np.int32) if pr.size else None), "pfm_halo_exchange")

    def check_finite(self, data_ptr: int, n: int):
        self._check(self.lib.pfm_check_finite(self._h, C.c_void_p(data_ptr), C.c_int64(n)), "pfm_check_finite")

    def state_set_device(self, sol_ptr: int, old_ptr: int, oldold_ptr: int):
        self._check(self.lib.pfm_state_set(self._h, C.c_void_p(sol_ptr), C.c_void_p(old_ptr),
                                           C.c_void_p(oldold_ptr), 1), "pfm_state_set")

    def state_set_solution_device(self, sol_ptr: int):
        """``pfm_state_set_solution``: old / old_old keep the values of the last full scatter (line search)."""
        self._check(self.lib.pfm_state_set_solution(self._h, C.c_void_p(sol_ptr), 1), "pfm_state_set_solution")

    def values_keep_uu_block(self, ptr: int):
        """``pfm_values_keep_uu_block``: promises that nothing but the library writes the (u,u) block at device address
        ``ptr``; assemblies into that pointer then leave it alone while old_solution, old_old_solution, the displacement
        constraints and the parameters are what they were when it was written.  Nothing is cleared.  Blocked layout only."""
        self._check(self.lib.pfm_values_keep_uu_block(self._h, C.c_void_p(ptr)), "pfm_values_keep_uu_block")

    def values_release_uu_block(self):
        """withdraws the promise of ``values_keep_uu_block`` (harmless without one)"""
        self._check(self.lib.pfm_values_keep_uu_block(self._h, None), "pfm_values_keep_uu_block")

    def values_uu_block_kept(self) -> int:
        """``pfm_values_uu_block_kept``: the device address of the kept (u,u) block, 0 if there is none."""
        p = C.c_void_p()
        self._check(self.lib.pfm_values_uu_block_kept(self._h, C.byref(p)), "pfm_values_uu_block_kept")
        return p.value or 0

    def state_set_host(self, sol: np.ndarray, old: np.ndarray, oldold: np.ndarray):
        a = [np.ascontiguousarray(x, np.float64) for x in (sol, old, oldold)]
        self._check(self.lib.pfm_state_set(self._h, capi.np_ptr(a[0], np.float64), capi.np_ptr(a[1], np.float64),
                                           capi.np_ptr(a[2], np.float64), 0), "pfm_state_set")

    def halo_register(self, send_ptr, send_nodes, recv_ptr, recv_nodes):
        sp = np.ascontiguousarray(send_ptr, np.int64)
        sn = np.ascontiguousarray(send_nodes, np.int32)
        rp = np.ascontiguousarray(recv_ptr, np.int64)
        rn = np.ascontiguousarray(recv_nodes, np.int32)
        self._check(self.lib.pfm_halo_register(self._h, sp.size - 1, capi.np_ptr(sp, np.int64),
                                               capi.np_ptr(sn, np.int32), capi.np_ptr(rp, np.int64),
                                               capi.np_ptr(rn, np.int32)), "pfm_halo_register")
        self.n_peers = int(sp.size - 1)  # contexts with peers have ghost nodes: no fused line-search call for them

    def halo_pack(self, peer: int, buf_ptr: int):
        self._check(self.lib.pfm_halo_pack(self._h, peer, C.c_void_p(buf_ptr)), "pfm_halo_pack")

    def halo_unpack(self, peer: int, buf_ptr: int):
        self._check(self.lib.pfm_halo_unpack(self._h, peer, C.c_void_p(buf_ptr)), "pfm_halo_unpack")

    def halo_pack_all(self, buf_ptr: int):
        self._check(self.lib.pfm_halo_pack_all(self._h, C.c_void_p(buf_ptr)), "pfm_halo_pack_all")

    def halo_unpack_all(self, buf_ptr: int):
        self._check(self.lib.pfm_halo_unpack_all(self._h, C.c_void_p(buf_ptr)), "pfm_halo_unpack_all")

    def assemble_device(self, residual_only: bool, value_ptrs: Sequence[int], res_pde_ptr: int, res_tot_ptr: int):
        arr = (C.c_void_p * 4)(*[C.c_void_p(p) for p in list(value_ptrs) + [0] * (4 - len(value_ptrs))])
        self._check(self.lib.pfm_assemble_device(self._h, 1 if residual_only else 0, arr,
                                                 C.c_void_p(res_pde_ptr), C.c_void_p(res_tot_ptr)),
                    "pfm_assemble_device")

    def assemble_nl_residual_device(self, sol_ptr: int, res_pde_ptr: int, res_tot_ptr: int):
        """``pfm_assemble_nl_residual_device``: solution := sol, then both residuals (the line-search call, cracks.cc:2942-2957);
        single-rank contexts only."""
        self._check(self.lib.pfm_assemble_nl_residual_device(self._h, C.c_void_p(sol_ptr), C.c_void_p(res_pde_ptr), C.c_void_p(res_tot_ptr)),
                    "pfm_assemble_nl_residual_device")

    def assemble_overlapped(self, comm_handle: int, peer_ranks, residual_only: bool, value_ptrs: Sequence[int], res_pde_ptr: int,
                            res_tot_ptr: int):
        """``pfm_assemble_overlapped``: ghost import on the context's side stream next to the interior tiles."""
        pr = np.ascontiguousarray(peer_ranks, np.int32)
        arr = (C.c_void_p * 4)(*[C.c_void_p(p) for p in list(value_ptrs) + [0] * (4 - len(value_ptrs))])
        self._check(self.lib.pfm_assemble_overlapped(self._h, C.c_void_p(comm_handle), capi.np_ptr(pr, np.int32) if pr.size else None,
                                                     1 if residual_only else 0, arr, C.c_void_p(res_pde_ptr),
                                                     C.c_void_p(res_tot_ptr)), "pfm_assemble_overlapped")

    def sync_status(self):
        self._check(self.lib.pfm_sync_status(self._h), "pfm_sync_status")

    def host_register(self, arr: np.ndarray):
        """``pfm_host_register``: page-lock a host array that ``assemble_host(..., out=...)`` reads or writes at every call.
        The caller keeps the array alive until ``host_unregister`` / ``close``."""
        self._check(self.lib.pfm_host_register(self._h, C.c_void_p(arr.ctypes.data), arr.nbytes), "pfm_host_register")

    def host_unregister(self, arr: np.ndarray = None):
        self._check(self.lib.pfm_host_unregister(self._h, C.c_void_p(arr.ctypes.data) if arr is not None else None), "pfm_host_unregister")

    def values_to_host(self, value_ptrs: Sequence[int], host_arrays: Sequence[np.ndarray]):
        """``pfm_values_to_host``: the device value blocks ``value_ptrs`` into the host arrays, synchronously."""
        dp = (C.c_void_p * 4)(*[C.c_void_p(p) for p in list(value_ptrs) + [0] * (4 - len(value_ptrs))])
        hp = (C.c_void_p * 4)(*[C.c_void_p(a.ctypes.data if a is not None and a.size else 0) for a in host_arrays])
        self._check(self.lib.pfm_values_to_host(self._h, dp, hp), "pfm_values_to_host")

    DELTA_STATS = ("bytes_moved", "bytes_total", "chunks_changed", "chunks", "slabs_direct", "slabs_packed")

    def values_to_host_delta(self, value_ptrs: Sequence[int], host_arrays: Sequence[np.ndarray]) -> dict:
        """``pfm_values_to_host_delta``: like ``values_to_host``, but only the chunks whose bits differ from what the last
        call left in ``host_arrays`` cross the link.  Returns the call's statistics: ``DELTA_STATS``, ``chunks_changed_block``
        (per block) and ``raw`` (the ten counters of the C ABI)."""
        dp = (C.c_void_p * 4)(*[C.c_void_p(p) for p in list(value_ptrs) + [0] * (4 - len(value_ptrs))])
        hp = (C.c_void_p * 4)(*[C.c_void_p(a.ctypes.data if a is not None and a.size else 0) for a in host_arrays])
        st = (C.c_int64 * 10)()
        self._check(self.lib.pfm_values_to_host_delta(self._h, dp, hp, st), "pfm_values_to_host_delta")
        raw = [int(x) for x in st]
        out = dict(zip(self.DELTA_STATS, raw[:6]))
        out["chunks_changed_block"] = raw[6:10]
        out["raw"] = raw
        return out

    def values_delta_reset(self):
        """``pfm_values_delta_reset``: the host wrote (zeroed, reallocated) its value arrays; the next delta call ships all."""
        self._check(self.lib.pfm_values_delta_reset(self._h), "pfm_values_delta_reset")

    def values_delta_config(self, chunk_bytes: int = 0, slab_bytes: int = 0):
        """tests and tuning: chunk and slab size of the delta transfer in bytes (0 = default); implies a reset."""
        self._check(self.lib.pfm_values_delta_config(self._h, int(chunk_bytes), int(slab_bytes)), "pfm_values_delta_config")

    def values_delta_info(self) -> dict:
        out = (C.c_int64 * 4)()
        self._check(self.lib.pfm_values_delta_info(self._h, out), "pfm_values_delta_info")
        return {"chunk_bytes": int(out[0]), "slab_bytes": int(out[1]), "device_bytes": int(out[2]), "valid": bool(out[3])}

    def values_keep_up_block(self, ptr: int):
        """``pfm_values_keep_up_block``: clears the (u,phi) block at device address ``ptr`` once (synchronous) and promises
        that nothing but the library writes it from here on; assemblies whose ``value_ptrs[1]`` is ``ptr`` then leave it
        untouched.  Blocked layout only.  Withdraw the promise (``values_release_up_block``, ``close``) before the array
        is freed."""
        self._check(self.lib.pfm_values_keep_up_block(self._h, C.c_void_p(ptr)), "pfm_values_keep_up_block")

    def values_release_up_block(self):
        """withdraws the promise of ``values_keep_up_block`` (harmless without one)"""
        self._check(self.lib.pfm_values_keep_up_block(self._h, None), "pfm_values_keep_up_block")

    def values_up_block_kept(self) -> int:
        """``pfm_values_up_block_kept``: the device address of the kept (u,phi) block, 0 if there is none."""
        p = C.c_void_p()
        self._check(self.lib.pfm_values_up_block_kept(self._h, C.byref(p)), "pfm_values_up_block_kept")
        return int(p.value or 0)

    def assemble_host(self, sol, old, oldold, residual_only: bool, out=None):
        """``pfm_assemble``: synchronous, host numpy in / host numpy out (single rank).  ``out`` = (values, res_pde,
        res_tot): arrays of an earlier call to write into again (what a host with its own matrix storage does; with
        ``host_register`` on them the transfers are DMA from page-locked memory)."""
        sol = np.ascontiguousarray(sol, np.float64)
        old = np.ascontiguousarray(old, np.float64)
        oldold = np.ascontiguousarray(oldold, np.float64)
        n = self.n_owned_dofs
        assert sol.size == old.size == oldold.size == n
        res_pde = out[1] if out is not None else np.zeros(n)
        res_tot = (out[2] if out is not None and out[2] is not None else np.zeros(n)) if residual_only else None
        values: List[np.ndarray] = []
        ptrs = (C.c_void_p * 4)()
        if not residual_only:
            for b in range(self.n_blocks):
                values.append(out[0][b] if out is not None else np.zeros(self.pattern_size(b)[1]))
                ptrs[b] = values[b].ctypes.data
        rc = self.lib.pfm_assemble(self._h, capi.np_ptr(sol, np.float64), capi.np_ptr(old, np.float64),
                                   capi.np_ptr(oldold, np.float64), 1 if residual_only else 0,
                                   None if residual_only else ptrs, capi.np_ptr(res_pde, np.float64),
                                   capi.np_ptr(res_tot, np.float64) if residual_only else None)
        self._check(rc, "pfm_assemble")
        return values, res_pde, res_tot

    def timing_enable(self, on: bool = True):
        self._check(self.lib.pfm_timing_enable(self._h, 1 if on else 0), "pfm_timing_enable")

    def kernel_time_ms(self):
        ms, n = C.c_double(), C.c_int()
        self._check(self.lib.pfm_kernel_time_ms(self._h, C.byref(ms), C.byref(n)), "pfm_kernel_time_ms")
        return ms.value, n.value

    def kernel_times_ms(self, capacity: int = 4096) -> np.ndarray:
        """Durations of the recorded launches (call before ``kernel_time_ms``, which resets the record)."""
        buf = np.zeros(capacity)
        n = C.c_int()
        self._check(self.lib.pfm_kernel_times_ms(self._h, capi.np_ptr(buf, np.float64), capacity, C.byref(n)), "pfm_kernel_times_ms")
        return buf[:min(n.value, capacity)]

    @property
    def kernel_path(self) -> int:
        return self.lib.pfm_ctx_kernel_path(self._h)

    def force_path(self, path: int):
        self._check(self.lib.pfm_ctx_force_path(self._h, path), "pfm_ctx_force_path")

    def overlay_info(self):
        """(rows written by the patch kernel of the cartesian overlay, cells left to the general family)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.pfm_ctx_overlay_info(self._h, C.byref(a), C.byref(b)), "pfm_ctx_overlay_info")
        return int(a.value), int(b.value)

    def force_phase(self, phase: int):
        """measurement: 1 / 2 = only the first / second half of the overlapped assembly, 0 = all."""
        self._check(self.lib.pfm_ctx_force_phase(self._h, phase), "pfm_ctx_force_phase")

    # marching kernels of pfm_ctx_force_zchunk / pfm_ctx_zchunk
    ZC_UU3, ZC_PHI4, ZC_RES3, ZC_RES2 = 0, 1, 2, 3

    def force_zchunk(self, kernel: int, planes: int):
        """tests and tuning: z-chunk length of a marching kernel (ZC_*), clamped to the plane count; 0 = the default."""
        self._check(self.lib.pfm_ctx_force_zchunk(self._h, kernel, planes), "pfm_ctx_force_zchunk")

    def zchunk(self, kernel: int) -> int:
        """the chunk length the next launch of the marching kernel over the context's box uses."""
        p = C.c_int(0)
        self._check(self.lib.pfm_ctx_zchunk(self._h, kernel, C.byref(p)), "pfm_ctx_zchunk")
        return int(p.value)

    @property
    def device_bytes(self) -> int:
        return int(self.lib.pfm_ctx_device_bytes(self._h))

    # ---- include/pfm_newton.h
    def diag_mass_device(self, mass_ptr: int):
        """cracks.cc:2514-2562 into a device vector over the owned nodes."""
        self._check(self.lib.pfm_diag_mass_device(self._h, C.c_void_p(mass_ptr)), "pfm_diag_mass_device")

    def active_set_device(self, res_tot_ptr: int, mass_ptr: int, c: float, sol_ptr: int, old_ptr: int, cycle_ptr: int):
        """cracks.cc:2837-2909; returns (active, cycling, changed)."""
        counts = (C.c_int64 * 3)()
        self._check(self.lib.pfm_active_set_device(self._h, C.c_void_p(res_tot_ptr), C.c_void_p(mass_ptr), C.c_double(c),
                                                   C.c_void_p(sol_ptr), C.c_void_p(old_ptr), C.c_void_p(cycle_ptr), counts),
                    "pfm_active_set_device")
        return int(counts[0]), int(counts[1]), int(counts[2])

    # ---- include/pfm_newton.h, the active-set update of a rank with ghost peers
    def active_set_owned_device(self, res_tot_ptr: int, mass_ptr: int, c: float, sol_ptr: int, old_ptr: int, cycle_ptr: int):
        """``pfm_active_set_owned_device``: ``active_set_device`` without the distribution of the hanging nodes, on any
        context (a partitioned one with hanging nodes too); returns (active, cycling, changed) of this rank."""
        counts = (C.c_int64 * 3)()
        self._check(self.lib.pfm_active_set_owned_device(self._h, C.c_void_p(res_tot_ptr), C.c_void_p(mass_ptr), C.c_double(c),
                                                         C.c_void_p(sol_ptr), C.c_void_p(old_ptr), C.c_void_p(cycle_ptr), counts),
                    "pfm_active_set_owned_device")
        return int(counts[0]), int(counts[1]), int(counts[2])

    def halo_pack_flags_all(self, buf_ptr: int):
        """``pfm_halo_pack_flags_all``: the flag bytes of the send nodes, one byte per node, peer k at byte send_ptr[k]."""
        self._check(self.lib.pfm_halo_pack_flags_all(self._h, C.c_void_p(buf_ptr)), "pfm_halo_pack_flags_all")

    def halo_unpack_flags_all(self, buf_ptr: int):
        """``pfm_halo_unpack_flags_all``: bit ``dim`` of the received bytes into the flag bytes of the ghost nodes."""
        self._check(self.lib.pfm_halo_unpack_flags_all(self._h, C.c_void_p(buf_ptr)), "pfm_halo_unpack_flags_all")

    def halo_exchange_flags(self, comm_handle: int, peer_ranks):
        """``pfm_halo_exchange_flags``: pack -> RCCL send/recv of the flag bytes -> unpack inside the library."""
        pr = np.ascontiguousarray(peer_ranks, np.int32)
        self._check(self.lib.pfm_halo_exchange_flags(self._h, C.c_void_p(comm_handle),
                                                     capi.np_ptr(pr, np.int32) if pr.size else None), "pfm_halo_exchange_flags")

    def distribute_hanging_device(self, sol_ptr: int = 0):
        """``pfm_distribute_hanging_device``: the hanging nodes of the node state, owned and ghost, from their parents'
        node values; owned ones also into the device dof vector ``sol_ptr`` (0: node arrays only)."""
        self._check(self.lib.pfm_distribute_hanging_device(self._h, C.c_void_p(sol_ptr)), "pfm_distribute_hanging_device")

    def active_set_exchange(self, comm_handle: int, peer_ranks, res_tot_ptr: int, mass_ptr: int, c: float, sol_ptr: int, old_ptr: int,
                            cycle_ptr: int):
        """``pfm_active_set_exchange``: cracks.cc:2826-2890 on a rank with ghost peers in one collective call (``comm_handle``
        0 and no ``peer_ranks`` on a context without peers); returns (active, cycling, changed) of this rank."""
        pr = np.ascontiguousarray(peer_ranks if peer_ranks is not None else [], np.int32)
        counts = (C.c_int64 * 3)()
        self._check(self.lib.pfm_active_set_exchange(self._h, C.c_void_p(comm_handle), capi.np_ptr(pr, np.int32) if pr.size else None,
                                                     C.c_void_p(res_tot_ptr), C.c_void_p(mass_ptr), C.c_double(c), C.c_void_p(sol_ptr),
                                                     C.c_void_p(old_ptr), C.c_void_p(cycle_ptr), counts), "pfm_active_set_exchange")
        return int(counts[0]), int(counts[1]), int(counts[2])

    def get_constraints(self) -> np.ndarray:
        flags = np.empty(self.n_nodes, np.uint8)
        self._check(self.lib.pfm_get_constraints(self._h, capi.np_ptr(flags, np.uint8)), "pfm_get_constraints")
        return flags

    def residual_norms(self, res_ptr: int):
        """(l2, linf, sum of squares) of a device residual vector with the constrained lines zeroed -- what the Newton loop
        and the line search read after every assembly (cracks.cc:2791-2794, 2947-2949); this rank's owned dofs."""
        out = (C.c_double * 3)()
        self._check(self.lib.pfm_residual_norms(self._h, C.c_void_p(res_ptr), out), "pfm_residual_norms")
        return float(out[0]), float(out[1]), float(out[2])

    # ---- include/pfm_newton.h, the line search
    LS_NORMS = {"l2": capi.LS_NORM_L2, "linf": capi.LS_NORM_LINF}
    LS_RESTORES = {"saved": capi.LS_RESTORE_SAVED, "subtract": capi.LS_RESTORE_SUBTRACT}

    def line_search_advance(self, sol_ptr: int, update_ptr: int, saved_ptr: int = 0):
        """``pfm_line_search_advance``: ``saved = solution`` (``saved_ptr`` != 0), ``solution = solution + update``."""
        self._check(self.lib.pfm_line_search_advance(self._h, C.c_void_p(sol_ptr), C.c_void_p(update_ptr), C.c_void_p(saved_ptr)),
                    "pfm_line_search_advance")

    def line_search_retreat(self, restore, damping: float, sol_ptr: int, update_ptr: int, saved_ptr: int = 0, advance: bool = False):
        """``pfm_line_search_retreat``: the restore of a rejected trial (``"saved"``: ``solution = saved``, ``"subtract"``:
        ``solution = solution - update``), ``update = update * damping`` and, with ``advance``, the next
        ``solution = solution + update`` in the same pass.  Every operation is rounded on its own."""
        mode = self.LS_RESTORES.get(restore, restore)
        self._check(self.lib.pfm_line_search_retreat(self._h, int(mode), float(damping), C.c_void_p(sol_ptr), C.c_void_p(update_ptr),
                                                     C.c_void_p(saved_ptr), 1 if advance else 0), "pfm_line_search_retreat")

    def line_search_device(self, sol_ptr: int, update_ptr: int, res_pde_ptr: int, res_tot_ptr: int, reference: float, max_steps: int,
                           damping: float, norm="l2", restore="saved") -> dict:
        """``pfm_line_search_device``: the whole line search (cracks.cc:2942-2957 / 3048-3062) on device vectors; contexts
        without halo peers.  Returns ``steps``, ``accepted``, ``norms`` (l2, linf, sum of squares of the last trial's
        residual_pde) and ``linf_block`` (displacement, phase field)."""
        o = capi.PfmLineSearchOpts(int(max_steps), int(self.LS_NORMS.get(norm, norm)), int(self.LS_RESTORES.get(restore, restore)), 0,
                                   float(damping), float(reference))
        r = capi.PfmLineSearchResult()
        self._check(self.lib.pfm_line_search_device(self._h, C.byref(o), C.c_void_p(sol_ptr), C.c_void_p(update_ptr),
                                                    C.c_void_p(res_pde_ptr), C.c_void_p(res_tot_ptr), C.byref(r)), "pfm_line_search_device")
        return {"steps": int(r.steps), "accepted": bool(r.accepted), "norms": tuple(float(x) for x in r.norms),
                "linf_block": tuple(float(x) for x in r.linf_block)}

    def project_back_device(self, sol_ptr: int):
        """``pfm_project_back_device``: project_back_phase_field (cracks.cc:3111-3137) on the owned phase-field dofs."""
        self._check(self.lib.pfm_project_back_device(self._h, C.c_void_p(sol_ptr)), "pfm_project_back_device")

    def functionals(self, cell_owned: Optional[np.ndarray] = None, cell_lambda=None, cell_mu=None):
        """(bulk energy, crack energy, TCV) of the node state in the context (cracks.cc:3553-3701); optional per-cell
        Lame coefficients for the energy (the reference's heterogeneous case uses other ones than the assembly)."""
        out = (C.c_double * 3)()
        mask = None if cell_owned is None else np.ascontiguousarray(cell_owned, np.uint8)
        mp = None if mask is None else capi.np_ptr(mask, np.uint8)
        if cell_lambda is None:
            self._check(self.lib.pfm_functionals(self._h, mp, out), "pfm_functionals")
        else:
            la = np.ascontiguousarray(cell_lambda, np.float64)
            mu = np.ascontiguousarray(cell_mu, np.float64)
            self._check(self.lib.pfm_functionals_material(self._h, mp, capi.np_ptr(la, np.float64),
                                                          capi.np_ptr(mu, np.float64), out), "pfm_functionals_material")
        return float(out[0]), float(out[1]), float(out[2])

    def face_load(self, cells, faces) -> np.ndarray:
        """Raw ``int_face sigma(u) n dA`` summed over the (cell, face) pairs (compute_load, cracks.cc:3726-3790), global Lame
        coefficients, no sign flips; this rank's part.  Returns a vector of ``dim`` entries."""
        c = np.ascontiguousarray(cells, np.int32)
        f = np.ascontiguousarray(faces, np.uint8)
        if c.shape != f.shape:
            raise ValueError("cells and faces differ in length")
        out = (C.c_double * 3)()
        self._check(self.lib.pfm_face_load(self._h, c.size, capi.np_ptr(c, np.int32), capi.np_ptr(f, np.uint8), out),
                    "pfm_face_load")
        return np.array(out[:self.dim])

    def cod_lines(self, lines, cell_owned: Optional[np.ndarray] = None, eps: float = 1e-8):
        """compute_cod of every line at once (cracks.cc:3453-3550): ``(cod, n_faces)``, the raw sums of this rank BEFORE
        the reference's ``/2`` and MPI sum.  The (line, cell, face) list is cached in the context for the same lines, eps
        and mask."""
        ln = np.ascontiguousarray(lines, np.float64)
        cod = np.zeros(ln.size)
        nf = np.zeros(ln.size, np.int64)
        mask = None if cell_owned is None else np.ascontiguousarray(cell_owned, np.uint8)
        mp = None if mask is None else capi.np_ptr(mask, np.uint8)
        self._check(self.lib.pfm_cod_lines(self._h, mp, ln.size, capi.np_ptr(ln, np.float64), float(eps),
                                           capi.np_ptr(cod, np.float64), capi.np_ptr(nf, np.int64)), "pfm_cod_lines")
        return cod, nf

    def sneddon_phi_error_sq(self, cell_owned: Optional[np.ndarray] = None) -> float:
        """``int (phi_h - phi_exact)^2`` of ExactPhiSneddon(alpha_eps) over this rank's cells (cracks.cc:4495-4516), before the
        MPI sum and the root."""
        out = (C.c_double * 1)()
        mask = None if cell_owned is None else np.ascontiguousarray(cell_owned, np.uint8)
        mp = None if mask is None else capi.np_ptr(mask, np.uint8)
        self._check(self.lib.pfm_sneddon_phi_error(self._h, mp, out), "pfm_sneddon_phi_error")
        return float(out[0])

    def cod_buckets(self, n_buckets: int = 75, x_lo: float = -1.5, x_hi: float = 1.5, n_sub: int = 100,
                    cell_owned: Optional[np.ndarray] = None):
        """compute_cod_array (cracks.cc:3337-3449) before its MPI sum: ``(values, volume)``, this rank's raw bucket sums of
        ``u . grad(phi) JxW`` and ``JxW`` over the ``n_sub^dim`` midpoints of every masked cell (``pfm_cod_buckets``)."""
        values, volume = np.zeros(max(int(n_buckets), 0)), np.zeros(max(int(n_buckets), 0))
        owned, mp = self._cell_bytes(cell_owned)  # (the array stays referenced across the call)
        self._check(self.lib.pfm_cod_buckets(self._h, mp, int(n_buckets), float(x_lo), float(x_hi), int(n_sub),
                                             capi.np_ptr(values, np.float64), capi.np_ptr(volume, np.float64)), "pfm_cod_buckets")
        return values, volume

    def point_eval(self, points, cell_owned: Optional[np.ndarray] = None):
        """``pfm_point_eval``: ``(cell [P], values [P, dim+1], grads [P, dim+1, dim])`` of the node state at the points
        ``[P, dim]``: the lowest-numbered masked cell that contains each point (-1: none, values and gradients 0), the Q1
        interpolant of (u, phi) and ``grads[p, c, d] = d(component c)/dx_d`` (cracks.cc:3264-3320)."""
        pts = np.ascontiguousarray(points, np.float64).reshape(-1, self.dim)
        n, nc = pts.shape[0], self.dim + 1
        cell = np.full(max(n, 1), -1, np.int32)  # (at least one entry: the pointers of an empty call are still valid)
        values, grads = np.zeros((max(n, 1), nc)), np.zeros((max(n, 1), nc, self.dim))
        buf = pts if n else np.zeros((1, self.dim))
        owned, mp = self._cell_bytes(cell_owned)
        self._check(self.lib.pfm_point_eval(self._h, mp, n, capi.np_ptr(buf, np.float64), capi.np_ptr(cell, np.int32),
                                            capi.np_ptr(values, np.float64), capi.np_ptr(grads, np.float64)), "pfm_point_eval")
        return cell[:n], values[:n], grads[:n]

    # ---- include/pfm_newton.h, mesh adaptation
    def refine_flags(self, phi_threshold: float = float("nan"), box_lo=None, box_hi=None, max_level: int = -1,
                     cell_owned: Optional[np.ndarray] = None, cell_level: Optional[np.ndarray] = None):
        """The refinement indicator of refine_mesh() (cracks.cc:3902-4116) on the node state in the context:
        ``(flags uint8 [n_cells], n_flagged)`` of this rank.  ``box_lo`` / ``box_hi``: the closed box of the fixed
        pre-refinement strategies (``dim`` entries, +-inf for open sides; None = no box)."""
        crit = capi.PfmRefineCriteria()
        crit.phi_threshold = float(phi_threshold)
        crit.use_box = 0 if box_lo is None else 1
        if box_lo is not None:
            for d in range(self.dim):
                crit.box_lo[d], crit.box_hi[d] = float(box_lo[d]), float(box_hi[d])
        crit.max_level = int(max_level)
        n_cells = self.n_cells
        mask = None if cell_owned is None else np.ascontiguousarray(cell_owned, np.uint8)
        level = None if cell_level is None else np.ascontiguousarray(cell_level, np.uint8)
        for a in (mask, level):
            if a is not None and a.size != n_cells:
                raise ValueError("one entry per cell expected")
        flags = np.zeros(n_cells, np.uint8)
        n = C.c_int64(0)
        self._check(self.lib.pfm_refine_flags(self._h, C.byref(crit), None if mask is None else capi.np_ptr(mask, np.uint8),
                                              None if level is None else capi.np_ptr(level, np.uint8),
                                              capi.np_ptr(flags, np.uint8), C.byref(n)), "pfm_refine_flags")
        return flags, int(n.value)

    def _criteria(self, phi_threshold, box_lo, box_hi, max_level):
        crit = capi.PfmRefineCriteria()
        crit.phi_threshold = float(phi_threshold)
        crit.use_box = 0 if box_lo is None else 1
        if box_lo is not None:
            for d in range(self.dim):
                crit.box_lo[d], crit.box_hi[d] = float(box_lo[d]), float(box_hi[d])
        crit.max_level = int(max_level)
        return crit

    def _cell_bytes(self, a):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, np.uint8)
        if a.size != self.n_cells:
            raise ValueError("one entry per cell expected")
        return a, capi.np_ptr(a, np.uint8)

    def kelly_indicator(self, eta_ptr: int, component_mask: Optional[int] = None, cell_owned: Optional[np.ndarray] = None):
        """``pfm_kelly_indicator``: the Kelly indicator (cracks.cc:4074-4083) of the node state in the context into the device
        array ``eta_ptr`` [n_cells] of doubles, asynchronously.  ``component_mask``: bit c < dim = displacement c, bit dim =
        phi; None = the displacements, as the reference."""
        mask = (1 << self.dim) - 1 if component_mask is None else int(component_mask)
        if mask < 0 or mask >= 1 << 32:
            raise ValueError("component_mask does not fit an unsigned int")
        owned, mp = self._cell_bytes(cell_owned)  # (the array stays referenced across the call)
        self._check(self.lib.pfm_kelly_indicator(self._h, mp, mask, C.c_void_p(eta_ptr)), "pfm_kelly_indicator")

    def indicator_select(self, ind_ptr: int, k: int, cell_owned: Optional[np.ndarray] = None):
        """``pfm_indicator_select``: ``(threshold, n_above, n_equal)``, the k-th largest (1-based) of the device array
        ``ind_ptr`` [n_cells] over the masked cells, exactly."""
        t, counts = C.c_double(0.0), (C.c_int64 * 2)()
        owned, mp = self._cell_bytes(cell_owned)  # (the array stays referenced across the call)
        self._check(self.lib.pfm_indicator_select(self._h, C.c_void_p(ind_ptr), mp, int(k), C.byref(t), counts), "pfm_indicator_select")
        return float(t.value), int(counts[0]), int(counts[1])

    def indicator_count(self, ind_ptr: int, t: float, cell_owned: Optional[np.ndarray] = None):
        """``pfm_indicator_count``: ``(n_above, n_equal)`` of the masked entries of the device array against ``t`` -- what a
        distributed host sums over the ranks while it bisects for the global threshold."""
        counts = (C.c_int64 * 2)()
        owned, mp = self._cell_bytes(cell_owned)  # (the array stays referenced across the call)
        self._check(self.lib.pfm_indicator_count(self._h, C.c_void_p(ind_ptr), mp, float(t), counts), "pfm_indicator_count")
        return int(counts[0]), int(counts[1])

    def refine_flags_mix(self, top_fraction: float = 0.3, component_mask: Optional[int] = None, phi_threshold: float = float("nan"),
                         box_lo=None, box_hi=None, max_level: int = -1, cell_owned: Optional[np.ndarray] = None,
                         cell_level: Optional[np.ndarray] = None):
        """``pfm_refine_flags_mix``: RefinementStrategy::mix (cracks.cc:4043-4116) on the node state in the context:
        ``(flags uint8 [n_cells], n_flagged, threshold)``."""
        crit = self._criteria(phi_threshold, box_lo, box_hi, max_level)
        mask = (1 << self.dim) - 1 if component_mask is None else int(component_mask)
        if mask < 0 or mask >= 1 << 32:
            raise ValueError("component_mask does not fit an unsigned int")
        owned, op = self._cell_bytes(cell_owned)  # (the arrays stay referenced across the call)
        level, lp = self._cell_bytes(cell_level)
        flags = np.zeros(self.n_cells, np.uint8)
        n, t = C.c_int64(0), C.c_double(0.0)
        self._check(self.lib.pfm_refine_flags_mix(self._h, C.byref(crit), float(top_fraction), mask, op, lp,
                                                  capi.np_ptr(flags, np.uint8), C.byref(n), C.byref(t)), "pfm_refine_flags_mix")
        return flags, int(n.value), float(t.value)

    def min_cell_diameter(self, cell_owned: Optional[np.ndarray] = None) -> float:
        """``min_cell_diameter`` over this rank's cells (cracks.cc:3824-3835); +inf where no cell is masked."""
        out = C.c_double(0.0)
        mask = None if cell_owned is None else np.ascontiguousarray(cell_owned, np.uint8)
        if mask is not None and mask.size != self.n_cells:
            raise ValueError("one entry per cell expected")
        self._check(self.lib.pfm_min_cell_diameter(self._h, None if mask is None else capi.np_ptr(mask, np.uint8), C.byref(out)),
                    "pfm_min_cell_diameter")
        return float(out.value)

    def transfer_state(self, dst: "Context", parent_cell, child, src_ptrs: Sequence[int], dst_ptrs: Sequence[int]):
        """``pfm_state_transfer``: SolutionTransfer::interpolate for refinement (cracks.cc:4137-4159) of the device dof vectors
        ``src_ptrs`` of this context into ``dst_ptrs`` of ``dst``.  ``parent_cell`` / ``child``: one entry per cell of
        ``dst`` (child 255 = identical cell, else the deal.II child number)."""
        pc = np.ascontiguousarray(parent_cell, np.int32)
        ch = np.ascontiguousarray(child, np.uint8)
        if pc.size != dst.n_cells or ch.size != dst.n_cells or len(src_ptrs) != len(dst_ptrs):
            raise ValueError("one (parent, child) entry per cell of dst and as many destination as source vectors expected")
        n = len(src_ptrs)
        sp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in src_ptrs])
        dp = (C.c_void_p * max(n, 1))(*[C.c_void_p(p) for p in dst_ptrs])
        rc = self.lib.pfm_state_transfer(self._h, dst._h, capi.np_ptr(pc, np.int32), capi.np_ptr(ch, np.uint8), n, sp, dp)
        if rc != capi.PFM_OK:
            raise PfmError(rc, "pfm_state_transfer", self.lib.pfm_last_error(dst._h).decode())


class Assembler:
    """Device-resident counterpart of the reference's assembly members.

    ``solution`` / ``old_solution`` / ``old_old_solution`` are torch device vectors over
    the owned dofs; ``assemble_system`` / ``assemble_nl_residual`` fill
    ``system_pde_matrix`` (list of CSR value vectors, one per block),
    ``system_pde_residual`` and ``system_total_residual`` on the device, asynchronously
    on torch's current stream."""

    def __init__(self, mesh, blocked: bool, device: int = 0, n_owned_nodes: Optional[int] = None,
                 cell_lambda=None, cell_mu=None, halo=None):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("cracks_amd.Assembler needs a ROCm GPU (there is no CPU fallback)")
        self.torch = torch
        self.dev = torch.device("cuda", device)
        torch.cuda.set_device(self.dev)
        self.ctx = Context(mesh, blocked, device, n_owned_nodes, cell_lambda, cell_mu)
        self.ctx.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        n = self.ctx.n_owned_dofs
        z = lambda: torch.zeros(n, dtype=torch.float64, device=self.dev)
        self.solution, self.old_solution, self.old_old_solution = z(), z(), z()
        self.system_pde_residual, self.system_total_residual = z(), z()
        self._system_pde_matrix: List = []
        self.halo = halo

    @property
    def system_pde_matrix(self) -> List:
        return self._system_pde_matrix

    @system_pde_matrix.setter
    def system_pde_matrix(self, blocks):
        # the promise on the (u,phi) block of allocate_matrix goes before the tensors do: the caching allocator may hand
        # the address to someone else.  Only that promise: one the caller gave for an array of its own
        # (ctx.values_keep_up_block) stays
        if (self._system_pde_matrix and self._keeps_up_block()
                and self.ctx.values_up_block_kept() == self._system_pde_matrix[1].data_ptr() != 0):
            self.ctx.values_release_up_block()
        if (self._system_pde_matrix and self._keeps_uu_block()
                and self.ctx.values_uu_block_kept() == self._system_pde_matrix[0].data_ptr() != 0):
            self.ctx.values_release_uu_block()
        self._system_pde_matrix = list(blocks) if blocks else []

    def _keeps_up_block(self) -> bool:
        # (PFM_LIB may name an older build in an A/B run)
        return self.ctx.n_blocks == 4 and hasattr(self.ctx.lib, "pfm_values_keep_up_block") and bool(getattr(self.ctx, "_h", None))

    def _keeps_uu_block(self) -> bool:
        return self.ctx.n_blocks == 4 and hasattr(self.ctx.lib, "pfm_values_keep_uu_block") and bool(getattr(self.ctx, "_h", None))

    @property
    def split_model(self) -> int:
        """The law of a stress-split assembly (Context.set_split_model): 0 the reference's closed form, 1 the spectral split of
        3-D meshes, 3 their volumetric-deviatoric split.  Set it before set_params."""
        return self.ctx.split_model

    @split_model.setter
    def split_model(self, model: int):
        self.ctx.set_split_model(model)

    @property
    def split_route(self) -> int:
        """Where the residual-only assembly of a 3-D mesh under a split law runs (Context.set_split_route): 0 the general
        family, 1 the row-owner kernels of the lattice under model 3, 3 under models 1 and 3; 5 and 7: the same, and the full
        assembly of model 3 on the row-owner kernels too; 13 and 15: also on the level lattices of a 3-D overlay; 21 and 23: 5 and 7 with
        the law evaluated only at compressed cells (boxes); 61 and 63: 13 and 15 likewise, on the level lattices too.  May change at
        any time."""
        return self.ctx.split_route

    @split_route.setter
    def split_route(self, route: int):
        self.ctx.set_split_route(route)

    @property
    def hanging_mode(self) -> int:
        """How the cells at hanging vertices reach the outputs (Context.set_hanging_mode): 0 the default, 1 scratch + ordered
        gather wherever a form exists (bitwise reproducible), 2 the atomic class.  May change at any time."""
        return self.ctx.hanging_mode

    @hanging_mode.setter
    def hanging_mode(self, mode: int):
        self.ctx.set_hanging_mode(mode)

    def allocate_matrix(self, keep_up_block: bool = False):
        """The value vectors, once.  ``keep_up_block`` (blocked layout; what ``assemble_system`` passes when it allocates
        them itself): the structurally zero (u,phi) block is cleared here and kept (Context.values_keep_up_block) -- the
        tensors are this object's own and nothing but the library writes them; a caller who does write
        ``system_pde_matrix[1]`` afterwards calls ``ctx.values_release_up_block()`` first.  A caller who allocates the
        matrix itself takes the tensors in hand before the first assembly, may prefill them, and gets no promise.

        Two consequences.  (1) After ``assemble_system`` has allocated the matrix, whatever a caller writes into
        ``system_pde_matrix[1]`` without withdrawing the promise STAYS there: the next assembly does not overwrite it
        (a caller that refills every block between assemblies allocates the matrix itself for that reason).
        (2) Callers that allocate first run unkept and measure the kernels that write the block; they pass
        ``keep_up_block=True`` to run the kept form.  A promise the caller has given the context for an array of its own
        is left in place."""
        if not self._system_pde_matrix:
            t = self.torch
            self._system_pde_matrix = [t.empty(self.ctx.pattern_size(b)[1], dtype=t.float64, device=self.dev)
                                       for b in range(self.ctx.n_blocks)]
            # (on the context's stream: assemble_system has set it to torch's current one)
            if (keep_up_block and self._keeps_up_block() and self._system_pde_matrix[1].numel() > 0
                    and self.ctx.values_up_block_kept() == 0):
                self.ctx.values_keep_up_block(self._system_pde_matrix[1].data_ptr())
            # ... and the (u,u) block is kept while the lagged phase field, the displacement constraints and the parameters
            # stay what they were (Context.values_keep_uu_block): given exactly where the other promise is
            if (keep_up_block and self._keeps_uu_block() and self._system_pde_matrix[0].numel() > 0
                    and self.ctx.values_uu_block_kept() == 0):
                self.ctx.values_keep_uu_block(self._system_pde_matrix[0].data_ptr())

    def set_params(self, prm):
        self.ctx.set_params(prm)

    def set_constraints(self, node_flags: np.ndarray):
        self.ctx.set_constraints(node_flags)

    def set_vectors(self, sol: np.ndarray, old: np.ndarray, oldold: np.ndarray):
        t = self.torch
        self.solution.copy_(t.from_numpy(np.ascontiguousarray(sol)))
        self.old_solution.copy_(t.from_numpy(np.ascontiguousarray(old)))
        self.old_old_solution.copy_(t.from_numpy(np.ascontiguousarray(oldold)))

    def assemble_system(self, residual_only: bool = False, solution_only: bool = False):
        """cracks.cc:2129-2475 (without the AMG set-up that follows it).  ``solution_only``: only ``solution`` changed
        since the last call (the line search of cracks.cc:2942-2957 and the Newton iterations within a time step):
        old_solution / old_old_solution are not scattered again."""
        self.ctx.set_stream(self.torch.cuda.current_stream(self.dev).cuda_stream)
        if solution_only and residual_only and self.halo is None and getattr(self.ctx, "n_peers", 0) == 0:
            # one library call; on a single-rank box the residual kernel reads `solution` itself (no scatter launch).  The
            # context's own state decides, not this wrapper's: a caller may register peers with ctx.halo_register and move
            # the ghosts itself (pack / unpack), and pfm_assemble_nl_residual_device refuses such contexts
            self.ctx.assemble_nl_residual_device(self.solution.data_ptr(), self.system_pde_residual.data_ptr(),
                                                 self.system_total_residual.data_ptr())
            return
        if solution_only:
            self.ctx.state_set_solution_device(self.solution.data_ptr())
        else:
            self.ctx.state_set_device(self.solution.data_ptr(), self.old_solution.data_ptr(),
                                      self.old_old_solution.data_ptr())
        if not residual_only:
            self.allocate_matrix(keep_up_block=True)
        ptrs = [m.data_ptr() for m in self.system_pde_matrix] if not residual_only else []
        # PFM_OVERLAP=1: the ghost import on the context's side stream next to the interior tiles.  Off by default: on one
        # node the import is ~0.05 ms (pack + unpack 0.02 ms measured, ~7 messages of <= 0.6 MB over xGMI) while cutting
        # the first kernel into an interior and a boundary launch costs 0.12 ms at 8 ranks (profiles/r03/rank_share_w8.json)
        lib_comm = self.halo.library_comm(self.ctx) if (self.halo is not None and os.environ.get("PFM_OVERLAP") == "1") else None
        if lib_comm is not None:
            # one library call: exchange on the side stream || interior tiles, then the tiles that read ghost nodes
            self.ctx.assemble_overlapped(lib_comm, self.halo.peers, residual_only, ptrs, self.system_pde_residual.data_ptr(),
                                         self.system_total_residual.data_ptr())
            return
        if self.halo is not None:
            self.halo.exchange(self.ctx)
        self.ctx.assemble_device(residual_only, ptrs, self.system_pde_residual.data_ptr(), self.system_total_residual.data_ptr())

    def assemble_nl_residual(self, solution_only: bool = False):
        """cracks.cc:2507-2512."""
        self.assemble_system(True, solution_only)

    def line_search(self, update, reference: float, max_steps: int, damping: float, norm: str = "l2", restore: str = "saved") -> dict:
        """The line search of cracks.cc:2942-2957 (``norm="l2", restore="saved"``) / 3048-3062 (``"linf", "subtract"``) in one
        library call on ``solution``, ``system_pde_residual`` and ``system_total_residual``; ``update`` is a device vector
        like ``solution``.  ``solution`` and ``update`` are modified in place; the residuals are those of the last trial.
        Single-rank assemblers (no halo).  Synchronous."""
        self.ctx.set_stream(self.torch.cuda.current_stream(self.dev).cuda_stream)
        if self.halo is not None:
            raise PfmError(1, "Assembler.line_search", "a rank with ghost peers composes the loop from line_search_advance / _retreat")
        assert update.dtype == self.torch.float64 and update.is_contiguous() and update.numel() == self.solution.numel()
        return self.ctx.line_search_device(self.solution.data_ptr(), update.data_ptr(), self.system_pde_residual.data_ptr(),
                                           self.system_total_residual.data_ptr(), reference, max_steps, damping, norm, restore)

    def residual_norm(self, total: bool = False) -> float:
        """constraints_update.set_zero(residual); residual.l2_norm() (cracks.cc:2791-2794, 2947-2949) of the last assembly, without
        moving the vector: 24 bytes come back.  Synchronous (as the reference's call)."""
        r = self.system_total_residual if total else self.system_pde_residual
        return self.ctx.residual_norms(r.data_ptr())[0]

    def synchronize(self):
        """Wait for the stream and raise what the reference would have thrown/aborted on."""
        self.ctx.sync_status()
