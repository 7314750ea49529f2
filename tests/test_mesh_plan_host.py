"""The mesh analysis of the context build (cracks_amd/csrc/pfm_mesh_plan.cpp on pfm_host_pool.cpp) as a stand-alone host
program under AddressSanitizer and UBSan (tests/cpp/mesh_plan_main.cpp).  The files include no HIP header, so a plain host
compiler builds the program; it needs no GPU and is not loaded into Python.

Every mesh is written to a file, analysed once with PFM_HOST_THREADS=1 and once with 4, and the two result files must be
the same byte for byte and have the digest recorded in tests/golden/mesh_plan_digests.json (recorded from the functions as
they were when they were moved out of pfm_host.cpp, before anything in them was simplified).  Then the tables are checked
in numpy against definitions that do not come from the code under test: a serial greedy colouring by the same rule, the
structure of the colour classes, the atomic ring, the lattice tables, and what makes a node a regular row of the overlay.

Two deviations from the plain wording of "regular" are the behaviour of the code as it has always been, and the checks
say so where they apply: a 3-D regular node on a face of its level's lattice has fewer than eight cells (the positions
outside the box of the level's cells are empty), and the ring is defined over a cell's own vertices."""
import hashlib
import json
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import topology_cases as T
from cracks_amd import mesh as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cracks_amd", "csrc")
MAIN = os.path.join(ROOT, "tests", "cpp", "mesh_plan_main.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_plan_digests.json")
HOST_FILES = ("pfm_host_pool.h", "pfm_host_pool.cpp", "pfm_mesh_plan.h", "pfm_mesh_plan.cpp")
MAX_COLOURS, MAX_RESOLVED = 62, 16
OVERFLOW = ("fan2d_closed64", "fan2d_open126", "fan2d_closed127", "fan3d_41", "fan3d_42", "fan3d_41_hanging")  # a node of more than 62 cells


def test_host_files_include_no_hip_header():
    allowed = {'"../../include/pfm_assemble.h"', '"pfm_switches.h"', '"pfm_host_pool.h"', '"pfm_mesh_plan.h"'}
    for name in HOST_FILES:
        text = open(os.path.join(CSRC, name)).read()
        includes = [ln.split()[1] for ln in text.splitlines() if ln.lstrip().startswith("#include")]
        assert includes, name
        for inc in includes:
            assert "hip" not in inc and "pfm_internal" not in inc, (name, inc)
            assert inc.startswith("<") or inc in allowed, (name, inc)


# ---- meshes --------------------------------------------------------------------------------------------------------------
def _renumbered(mesh, seed):
    """the same mesh with nodes and cells in a seeded random order (new id of node n: perm[n])"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(mesh.n_nodes)
    coords = np.empty_like(mesh.coords)
    coords[perm] = mesh.coords
    cells = perm[mesh.cells][rng.permutation(mesh.n_cells)].astype(np.int32)
    return M.Mesh(dim=mesh.dim, coords=coords, cells=np.ascontiguousarray(cells), box_shape=mesh.box_shape)


def _refined_patch(dim, n, lo, hi):
    """a box of n cells whose cells with their centre in [lo, hi]^dim are refined once"""
    m = M.box_mesh(dim, n)
    c = m.coords[m.cells].mean(axis=1)
    return M.refine_cells(m, ((c > lo) & (c < hi)).all(axis=1))


def _moved(mesh):
    m = M.Mesh(dim=mesh.dim, coords=mesh.coords.copy(), cells=mesh.cells, box_shape=mesh.box_shape)
    m.coords[m.n_nodes // 2, 0] += 1e-3
    return m


def _overlay3d_mesh():
    from test_gpu_overlay3d import refined_block_case
    return refined_block_case((12, 10, 12), True).mesh


def _het(mesh):
    rng = np.random.default_rng(11)
    mu = rng.uniform(0.5, 3.0, mesh.n_cells)
    return mesh, {"material": (0.4 * mu, mu)}


# name -> () -> mesh, or (mesh, options); options: owned (count), material ((lambda, mu) per cell)
MESHES = {make.__name__: (lambda make=make: make().mesh) for make in T.ALL}
MESHES.update({
    "sneddon_2d": M.sneddon_2d_prerefined_mesh,
    "sneddon_2d_ghosts": lambda: (M.sneddon_2d_prerefined_mesh(), {"owned": 100}),
    "slit": M.slit_mesh,
    "hetero_3d": lambda: _het(M.hetero_3d_prerefined_mesh()),
    "overlay3d_block": _overlay3d_mesh,
    "overlay3d_block_ghosts": lambda: (_overlay3d_mesh(), {"owned": 2000}),
    "hang3d": T.hang3d_mesh,
    "box2d": lambda: M.box_mesh(2, (9, 7)),
    "box2d_permuted": lambda: _renumbered(M.box_mesh(2, (9, 7)), 1),
    "box3d_permuted": lambda: _renumbered(M.box_mesh(3, (5, 4, 3)), 2),
    "box2d_node_moved": lambda: _moved(M.box_mesh(2, (9, 7))),
    "box3d_node_moved": lambda: _moved(M.box_mesh(3, (5, 4, 3))),
    # two chunks and more at four threads in every chunked loop (grains: 8192 and 16384 items, 65536 cells)
    "large2d_refined": lambda: _refined_patch(2, (368, 360), -1.5, 1.5),
    "large2d_box_permuted": lambda: _renumbered(M.box_mesh(2, (368, 360)), 3),
    "large3d_refined": lambda: _refined_patch(3, 28, -4.0, 4.0),
})
# the least number of blocks (2-D) or level lattices (3-D) of the meshes that are here for their overlay: one; both levels
# of a box with a refined block; two chunks of the block loop (its grain is 64 blocks)
OVERLAY = {"sneddon_2d": 1, "slit": 1, "hetero_3d": 1, "overlay3d_block": 2, "large3d_refined": 2, "large2d_refined": 128}
LATTICES = ("box2d", "box2d_permuted", "box3d_permuted", "large2d_box_permuted")


# ---- the program ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host compiler")
    exe = str(tmp_path_factory.mktemp("mesh_plan") / "mesh_plan_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                           "-I" + CSRC, MAIN, os.path.join(CSRC, "pfm_mesh_plan.cpp"), os.path.join(CSRC, "pfm_host_pool.cpp"), "-o", exe])
    return exe


def _write_mesh(path, mesh, owned=None, material=None):
    box = list(mesh.box_shape or ()) + [0, 0, 0]
    head = [mesh.dim, mesh.n_nodes, mesh.n_nodes if owned is None else owned, mesh.n_cells, mesh.hn_nodes.size, box[0], box[1], box[2],
            mesh.hn_parents.size, 0 if material is None else 1]
    with open(path, "wb") as f:
        f.write(np.asarray(head, np.int64).tobytes())
        for a, t in ((mesh.cells, np.int32), (mesh.coords, np.float64), (mesh.hn_nodes, np.int32), (mesh.hn_ptr, np.int64),
                     (mesh.hn_parents, np.int32)) + (() if material is None else ((material[0], np.float64), (material[1], np.float64))):
            f.write(np.ascontiguousarray(a, t).tobytes())


def _read_result(raw):
    out, at = {}, 0
    types = {b"B": np.uint8, b"b": np.int8, b"i": np.int32, b"q": np.int64, b"d": np.float64}
    while at < len(raw):
        (nl,) = struct.unpack_from("<I", raw, at)
        name = raw[at + 4:at + 4 + nl].decode()
        t = types[raw[at + 4 + nl:at + 5 + nl]]
        (cnt,) = struct.unpack_from("<q", raw, at + 5 + nl)
        at += 13 + nl
        out[name] = np.frombuffer(raw, t, cnt, at)
        at += cnt * np.dtype(t).itemsize
    return out


def _run(program, tmp_path, mesh, **options):
    """the result file at 1 and at 4 host threads"""
    _write_mesh(tmp_path / "mesh.bin", mesh, **options)
    raws = []
    for threads in (1, 4):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PFM_")}
        env["PFM_HOST_THREADS"] = str(threads)
        r = subprocess.run([program, str(tmp_path / "mesh.bin"), str(tmp_path / "plan.bin")], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout + r.stderr
        raws.append(open(tmp_path / "plan.bin", "rb").read())
        if b"mesh_plan" in r.stdout.encode():
            assert f"mesh_plan: OK threads={threads}" in r.stdout
    return raws


# ---- definitions, independent of the code under test ---------------------------------------------------------------------
def _resolved(cells, hn, hn_ptr, hn_parents):
    """per cell at a hanging vertex: its distinct constraint-resolved nodes, in vertex order"""
    out = {}
    for k in np.nonzero((hn[cells] >= 0).any(axis=1))[0]:
        r = []
        for n in cells[k]:
            line = hn[n]
            for p in ([int(n)] if line < 0 else hn_parents[hn_ptr[line]:hn_ptr[line + 1]]):
                if int(p) not in r:
                    r.append(int(p))
        out[int(k)] = r
    return out


def _greedy(cells, n_nodes, hn, resolved, subset):
    """Serial greedy colouring: the lowest colour free at all nodes of the cell -- its vertices, or its resolved nodes
    (resolved is not None: coloured-hanging mode).  A cell at a hanging vertex (plain mode), with more than 16 resolved nodes,
    or without a colour below 62 goes to the last class.  Returns the class of every cell (-1: not in the subset, n_col: last
    class), n_col, and whether a cell that could have had a colour found none."""
    used = [0] * n_nodes
    col = np.full(cells.shape[0], -1)
    atomic, overflow = [], False
    hanging = (hn[cells] >= 0).any(axis=1) if hn is not None else np.zeros(cells.shape[0], bool)
    rows = cells.tolist()
    for k in (range(len(rows)) if subset is None else np.nonzero(subset)[0].tolist()):
        nodes = rows[k]
        colourable = not hanging[k]
        if hanging[k] and resolved is not None:
            nodes = resolved[k]
            colourable = len(nodes) <= MAX_RESOLVED
        c = 63
        if colourable:
            mask = 0
            for n in nodes:
                mask |= used[n]
            free = ~mask & (2 ** 64 - 1)
            c = (free & -free).bit_length() - 1 if free else 63
        if c < MAX_COLOURS:
            for n in nodes:
                used[n] |= 1 << c
            col[k] = c
        else:
            atomic.append(k)
            overflow = overflow or colourable
    n_col = int(col.max()) + 1
    col[atomic] = n_col
    return col, n_col, overflow


def _check_colours(res, pre, cells, n_nodes, hn, resolved, subset, expect_overflow=None):
    ptr, order = res[pre + "_ptr"], res[pre + "_order"]
    col, n_col, overflow = _greedy(cells, n_nodes, hn, resolved, subset)
    # the same sequence of colours as the serial colouring
    listed = np.nonzero(col >= 0)[0]
    assert ptr.size == n_col + 2 and ptr[0] == 0
    assert np.array_equal(np.diff(ptr), np.bincount(col[listed], minlength=n_col + 1))
    assert np.array_equal(order, listed[np.argsort(col[listed], kind="stable")])
    assert bool(res[pre + "_overflow"][0]) == overflow
    if expect_overflow is not None:
        assert overflow == expect_overflow
    # class structure, without the serial colouring
    want = np.arange(cells.shape[0]) if subset is None else np.nonzero(subset)[0]
    assert np.array_equal(np.sort(order), want)  # a permutation of exactly the subset
    for c in range(n_col + 1):
        mine = order[ptr[c]:ptr[c + 1]]
        assert (np.diff(mine) > 0).all()  # ascending within a class
        if c < n_col:  # a plain class: no two cells share a resolved node
            if resolved is None:
                assert hn is None or (hn[cells[mine]] < 0).all()
                nodes = cells[mine].ravel()
            else:
                nodes = np.concatenate([resolved.get(int(k), cells[k]) for k in mine]) if mine.size else np.zeros(0, int)
                assert all(len(resolved.get(int(k), ())) <= MAX_RESOLVED for k in mine)
            assert np.unique(nodes).size == nodes.size
    if pre in ("col", "colh"):  # the same lists from the structure-of-arrays copy of the cell table
        assert res[pre + "_soa_same"][0] == 1


def _check_ring(res, pre, cells, n_nodes, hn, hn_ptr, hn_parents, resolved):
    """ring_cells: the cells of the plain classes that have a vertex which a cell of the atomic class (a cell at a hanging
    vertex; coloured-hanging mode: one with more than 16 resolved nodes) has as a vertex or as a parent of a vertex"""
    ring, any_ring = res[pre + "_ring"], bool(res[pre + "_ring_any"][0])
    assert res[pre + "_ring_soa_same"][0] == 1
    if hn is None:
        assert not any_ring and ring.size == 0
        return
    at_hanging = (hn[cells] >= 0).any(axis=1)
    if resolved is not None:
        at_hanging &= np.array([len(resolved.get(k, ())) > MAX_RESOLVED for k in range(cells.shape[0])])
    touched = np.zeros(n_nodes, bool)
    v = cells[at_hanging].ravel()
    touched[v] = True
    for line in hn[v][hn[v] >= 0]:
        touched[hn_parents[hn_ptr[line]:hn_ptr[line + 1]]] = True
    want = ~at_hanging & touched[cells].any(axis=1)
    assert any_ring == bool(want.any())
    assert (ring.size == 0) == (not any_ring)  # empty exactly when the function returns false
    if any_ring:
        assert np.array_equal(ring.astype(bool), want)


def _check_lattice(res, mesh, owned):
    dim, X = mesh.dim, mesh.coords
    NX, NY, NZ = (int(q) for q in res["lat_dims"][:3])
    nc = [int(q) for q in res["lat_dims"][3:]]
    assert [NX, NY, NZ][:dim] == [n + 1 for n in mesh.box_shape] and nc[:dim] == list(mesh.box_shape)
    lob, bol = res["local_of_box"], res["box_of_local"]
    assert lob.size == bol.size == mesh.n_nodes and np.array_equal(lob[bol], np.arange(mesh.n_nodes)) and np.array_equal(bol[lob], np.arange(mesh.n_nodes))
    idx = np.stack([bol % NX, (bol // NX) % NY, bol // (NX * NY)], axis=1)[:, :dim]
    h = res["lat_h"][:dim]
    assert np.allclose(h, (X.max(axis=0) - X.min(axis=0)) / np.asarray(mesh.box_shape), rtol=1e-15, atol=0)
    assert np.abs(X - (X.min(axis=0) + idx * h)).max() <= 1e-9 * h.min()  # node coordinates = origin + index x h
    # rows: the lattice offsets inside the box, in offset order
    ijk = np.stack([bol % NX, (bol // NX) % NY, bol // (NX * NY)], axis=1)[:owned].astype(np.int64)
    no = 27 if dim == 3 else 9
    o = np.arange(no)
    off = np.stack([o % 3 - 1, (o // 3) % 3 - 1, (o // 9 - 1) if dim == 3 else 0 * o], axis=1)
    nb = ijk[:, None, :] + off[None, :, :]
    valid = ((nb >= 0) & (nb < np.array([NX, NY, NZ]))).all(axis=2)
    ids = lob[np.where(valid, nb[..., 0] + NX * (nb[..., 1] + NY * nb[..., 2]), 0)]
    assert np.array_equal(res["lat_row_deg"], valid.sum(axis=1))
    assert np.array_equal(res["lat_row_mask"].view(np.uint32), (valid * (1 << o)).sum(axis=1).astype(np.uint32))
    assert np.array_equal(res["lat_rows"], ids[valid])
    # parity classes of the cells' lattice positions
    p = idx[mesh.cells[:, 0]] & 1
    col = p[:, 0] + 2 * p[:, 1] + (4 * p[:, 2] if dim == 3 else 0)
    n_col = 8 if dim == 3 else 4
    assert np.array_equal(np.diff(res["latcol_ptr"]), np.bincount(col, minlength=n_col + 1)) and res["latcol_ptr"][0] == 0
    assert np.array_equal(res["latcol_order"], np.argsort(col, kind="stable")) and res["latcol_overflow"][0] == 0


def _check_overlay(res, mesh, owned, hn, material):
    """what makes a node a regular row, the row split, and the block tables (2-D) or level lattices (3-D)"""
    dim, nv, X, cells, N = mesh.dim, mesh.nv, mesh.coords, mesh.cells, mesh.n_nodes
    regular, hang = res["regular"], res["hang"]
    if regular.size == 0:  # no overlay on this mesh
        assert int(res["n_regular"][0]) == 0 and res["rows_general"].size == 0 and "need" not in res
        assert int(res["n_blocks" if dim == 2 else "n_levels"][0]) == 0
        return False
    regular = regular.astype(bool)
    hanging = hn >= 0 if hn is not None else np.zeros(N, bool)
    parent = np.zeros(N, bool)
    parent[mesh.hn_parents] = True
    _, inverse, counts = np.unique(X, axis=0, return_inverse=True, return_counts=True)
    duplicated = counts[inverse.ravel()] > 1  # two nodes at one position (the lips of a slit)
    assert np.array_equal(hang.astype(bool), hanging | duplicated if dim == 2 else hanging)
    # the row split
    assert not regular[owned:].any() and int(res["n_regular"][0]) == regular.sum() > 0
    assert np.array_equal(res["rows_general"], np.nonzero(~regular[:owned])[0])
    # regular: owned, not hanging, not a parent
    assert not (regular & (hanging | parent | duplicated)).any()
    # ... its cells: at most one per corner, each an axis-parallel box with the node at that corner, all of one size, and no
    # hanging (or duplicated) node among their vertices, which are the 3^dim lattice neighbours
    size = X[cells[:, nv - 1]] - X[cells[:, 0]]
    corner = np.array([[(a >> d) & 1 for d in range(dim)] for a in range(nv)])
    scale = np.abs(X).max()
    is_box = (size > 0).all(axis=1) & (np.abs(X[cells] - (X[cells[:, 0]][:, None, :] + corner[None] * size[:, None, :])) <= 16 * 2.3e-16 * scale).all(axis=(1, 2))
    inc_n, inc_a = cells.ravel(), np.tile(np.arange(nv), cells.shape[0])
    inc_k = np.repeat(np.arange(cells.shape[0]), nv)
    sel = regular[inc_n]
    slot = np.bincount(inc_n[sel] * nv + inc_a[sel], minlength=N * nv).reshape(N, nv)
    assert slot.max() <= 1
    n_cells_at = slot.sum(axis=1)
    assert is_box[inc_k[sel]].all()
    assert not (hanging | duplicated)[cells[inc_k[sel]]].any()
    hmin, hmax = np.full((N, dim), np.inf), np.zeros((N, dim))
    np.minimum.at(hmin, inc_n[sel], size[inc_k[sel]])
    np.maximum.at(hmax, inc_n[sel], size[inc_k[sel]])
    assert (hmax[regular] - hmin[regular] <= 1e-9 * hmin[regular]).all()
    if dim == 2:
        assert (n_cells_at[regular] == 4).all()  # exactly 2^dim cells, one at each lattice position around the node
    # the reduced lists of the general family: the cells that touch a row the overlay does not write
    need = hang.astype(bool)[cells].any(axis=1) | ((cells < owned) & ~regular[cells]).any(axis=1)
    assert np.array_equal(res["need"].astype(bool), need)
    if dim == 2:
        nb = int(res["n_blocks"][0])
        bc, bn = res["blk_cells"].reshape(nb, 8, 8), res["blk_nodes"].reshape(nb, 9, 9)
        own = bn[:, 1:8, 1:8]
        own = own[own >= 0]
        own = own[(own < owned)]
        assert np.array_equal(np.bincount(own[regular[own]], minlength=N), regular.astype(int))  # an owned position of exactly one block
        # a block's nodes agree with its cells (an owned position may be blanked where a regular node of another level sits)
        want = np.full((nb, 9, 9), -1)
        for a in range(4):
            view = want[:, (a >> 1):(a >> 1) + 8, (a & 1):(a & 1) + 8]
            view[bc >= 0] = cells[bc[bc >= 0], a]
        differ = bn != want
        lips = differ & (bn >= 0)  # two nodes at one position: either cell's vertex may stand there
        assert (want[lips] >= 0).all() and duplicated[bn[lips]].all() and np.array_equal(X[bn[lips]], X[want[lips]])
        blank = differ & ~lips
        assert (want[blank] >= 0).all() and regular[want[blank]].all()
        assert (np.nonzero(blank)[1] % 8 > 0).all() and (np.nonzero(blank)[2] % 8 > 0).all()  # an owned position
    else:
        nl = int(res["n_levels"][0])
        seen = np.zeros(N, int)
        xmin = X.min(axis=0)
        for l in range(nl):
            dims, lo, h = res[f"lv{l}_dims"], res[f"lv{l}_lo"], res[f"lv{l}_h"]
            node_at, row_at = res[f"lv{l}_node_at"], res[f"lv{l}_row_at"]
            assert node_at.size == row_at.size == dims.prod()
            at = np.nonzero(row_at >= 0)[0]
            assert regular[row_at[at]].all() and np.array_equal(row_at[at], node_at[at]) and at.size == res[f"lv{l}_n_rows"][0]
            np.add.at(seen, row_at[at], 1)
            # the node at a lattice position lies there
            p = np.nonzero(node_at >= 0)[0]
            ijk = np.stack([p % dims[0], (p // dims[0]) % dims[1], p // (dims[0] * dims[1])], axis=1)
            assert np.abs(X[node_at[p]] - (xmin + (lo + ijk) * h)).max() <= 1e-6 * h.min()
            # a regular node with fewer than eight cells lies on a face of its level's lattice
            mine = row_at[at]
            pos = np.stack([at % dims[0], (at // dims[0]) % dims[1], at // (dims[0] * dims[1])], axis=1)
            on_face = ((pos == 0) | (pos == dims - 1)).any(axis=1)
            assert (n_cells_at[mine][~on_face] == 8).all() and (n_cells_at[mine] >= 1).all()
            if material is not None:
                cl = np.nonzero((np.abs(size - h) <= 1e-9 * h).all(axis=1) & is_box)[0]
                q = np.rint((X[cells[cl, 0]] - xmin) / h).astype(np.int64) - lo
                inside = ((q >= 0) & (q < dims - 1)).all(axis=1)
                flat = q[inside, 0] + (dims[0] - 1) * (q[inside, 1] + (dims[1] - 1) * q[inside, 2])
                assert np.array_equal(res[f"lv{l}_lam"][flat], material[0][cl[inside]]) and np.array_equal(res[f"lv{l}_mu"][flat], material[1][cl[inside]])
        assert np.array_equal(seen, regular.astype(int))  # every regular node in exactly one level
    return True


# ---- the tests -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MESHES))
def test_mesh_plan(program, tmp_path, name):
    made = MESHES[name]()
    mesh, options = made if isinstance(made, tuple) else (made, {})
    owned, material = options.get("owned", mesh.n_nodes), options.get("material")
    one, four = _run(program, tmp_path, mesh, **options)
    assert one == four, "the plan depends on the number of host threads"
    digest = hashlib.sha256(one).hexdigest()
    print(f'  "{name}": "{digest}",')
    assert json.load(open(GOLDEN))[name] == digest
    res = _read_result(one)
    assert res["hn_error"].size == 0 and res["cancelled"][0] == 1
    N, cells = mesh.n_nodes, mesh.cells
    hn = None
    if mesh.hn_nodes.size:
        hn = np.full(N, -1)
        hn[mesh.hn_nodes] = np.arange(mesh.hn_nodes.size)
        assert np.array_equal(res["hn_index"], hn)
    else:
        assert res["hn_index"].size == 0
    # lattice
    assert bool(res["lattice_ok"][0]) == (name in LATTICES)
    if name in LATTICES:
        _check_lattice(res, mesh, owned)
    # colour classes and ring, in both modes
    coloured = bool(res["hanging_coloured"][0])
    assert coloured == (mesh.dim == 3 and hn is not None and int(np.diff(mesh.hn_ptr).max()) <= 4)
    resolved = _resolved(cells, hn, mesh.hn_ptr, mesh.hn_parents) if hn is not None else None
    assert (name in OVERFLOW) == (np.bincount(cells.ravel()).max() > MAX_COLOURS)
    _check_colours(res, "col", cells, N, hn, None, None, expect_overflow=name in OVERFLOW)
    _check_ring(res, "col", cells, N, hn, mesh.hn_ptr, mesh.hn_parents, None)
    if coloured:
        _check_colours(res, "colh", cells, N, hn, resolved, None, expect_overflow=name in OVERFLOW)
        _check_ring(res, "colh", cells, N, hn, mesh.hn_ptr, mesh.hn_parents, resolved)
        if name == "hang3d_17resolved":  # the cell of more than 16 resolved nodes is the one cell left in the last class
            assert list(res["colh_order"][res["colh_ptr"][-2]:]) == [k for k, r in resolved.items() if len(r) > MAX_RESOLVED] != []
    # cells at hanging vertices
    if hn is not None:
        at_hanging = np.nonzero((hn[cells] >= 0).any(axis=1))[0]
        fits = int(np.diff(mesh.hn_ptr).max()) <= (4 if mesh.dim == 3 else 2)
        assert fits == (name not in ("hang2d_3parents", "hang3d_5parents"))
        assert bool(res["hcells_ok"][0]) == (fits and at_hanging.size > 0)
        if fits:
            assert np.array_equal(res["hcells"], at_hanging)
            place = np.full(mesh.n_cells, -1)
            place[at_hanging] = np.arange(at_hanging.size)
            assert np.array_equal(res["hcell"], place)
        else:
            assert res["hcells"].size == 0 and res["hcell"].size == 0
    # the overlay plan and the colour classes of the cells it leaves to the general family
    overlay = _check_overlay(res, mesh, owned, hn, material)
    if name in OVERLAY:  # (a plan that silently came out empty would pass every check on it)
        assert overlay and int(res["n_blocks" if mesh.dim == 2 else "n_levels"][0]) >= OVERLAY[name]
    if overlay:
        need = res["need"].astype(bool)
        _check_colours(res, "red", cells, N, hn, None, need)
        if coloured:
            _check_colours(res, "redh", cells, N, hn, resolved, need)


@pytest.mark.parametrize("what, text", [("node", "hn_nodes out of range"), ("parent", "hanging table must be closed (parents unconstrained)"),
                                        ("parent_range", "hanging table must be closed (parents unconstrained)")])
def test_hanging_table_errors(program, tmp_path, what, text):
    m = M.sneddon_2d_prerefined_mesh()
    if what == "node":
        m.hn_nodes = m.hn_nodes.copy()
        m.hn_nodes[3] = m.n_nodes
    else:
        m.hn_parents = m.hn_parents.copy()
        m.hn_parents[5] = m.hn_nodes[0] if what == "parent" else -1
    one, four = _run(program, tmp_path, m)
    assert one == four and bytes(_read_result(one)["hn_error"]).decode() == text
