"""GPU tests of the mesh dihedral angles (csrc/mesh_dihedral.hip through pytorch_points_amd/mesh_dihedral.py): the
(E,4) table bit for bit against the CPU build, its errors, the vertex lists, forward and backward against the fp64 CPU
composition within a bound measured on the fp32 CPU composition, the fixed values of a flat grid, run-to-run identity,
the reference-API names on CUDA tensors, graph capture and a side stream, and MeshDihedralAngleLoss."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from pytorch_points_amd import mesh_dihedral
from pytorch_points_amd.network import geo_operations, model_loss
from test_mesh_dihedral_host import (BOUNDARY, FLAT, HI, LO, assert_clear_of_the_clamp, folded_grid, jittered_cage,
                                     named_faces, swapped, table_of, two_topologies, zigzag_fan)
from test_mesh_edges_host import REDUCTIONS, fan_mesh, grid_mesh

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS32 = 2.0 ** -23


def dev_t(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda").requires_grad_(grad)


def cpu_table(faces):
    return mesh_dihedral.edge_points_composition(torch.from_numpy(faces)).numpy()


def assert_table(topo, b, want):
    """batch element b of topo: rows, padding and counts, bit for bit"""
    table = topo.edge_points[b].cpu().numpy()
    assert topo.counts_host[b] == want.shape[0] and int(topo.counts[b]) == want.shape[0]
    assert table.dtype == np.int64 and np.array_equal(table[:want.shape[0]], want)
    assert (table[want.shape[0]:] == -1).all()


# ------------------------------------------------------------------------------------------------- 1. the table
@pytest.mark.parametrize("name", ["tetrahedron", "grid_3x3", "grid_40x130", "fan_300", "fan_8000", "cage"])
def test_table_bit_equal_to_the_cpu_build(cuda, name):
    faces, n = named_faces(name)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), n)
    assert topo.batch == 1 and topo.edge_points.shape == (1, 3 * faces.shape[0], 4)
    want = cpu_table(faces)
    assert_table(topo, 0, want)
    if name != "fan_8000":
        assert np.array_equal(want, table_of(name))          # (and the CPU build is the independent one's)


def test_table_batch_of_two_topologies(cuda):
    _, faces = two_topologies()
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), 99)
    assert topo.batch == 2 and topo.counts_host == (258, 240)
    for b in range(2):
        assert_table(topo, b, cpu_table(faces[b]))
        assert np.array_equal(topo.table(b).cpu().numpy(), cpu_table(faces[b]))


def test_table_of_an_expanded_view_builds_once_and_int32_faces(cuda):
    faces, n = named_faces("grid_40x130")
    want = cpu_table(faces)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces)[None].expand(4, -1, -1), n)
    assert topo.batch == 1 and topo.count(3) == want.shape[0]
    assert_table(topo, 0, want)
    assert_table(mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces.astype(np.int32)), n), 0, want)


def test_three_builds_give_identical_bytes(cuda):
    faces, n = named_faces("fan_300")
    tf = dev_t(faces)
    runs = []
    for _ in range(3):
        topo = mesh_dihedral.MeshEdgePoints.from_faces(tf, n)
        start, entries = topo.incidence()
        total = int(start[0, -1])
        assert total == 4 * topo.count(0)
        runs.append((topo.edge_points.cpu().numpy().tobytes(), start.cpu().numpy().tobytes(),
                     entries[0, :total].cpu().numpy().tobytes()))
    assert runs[0] == runs[1] == runs[2]


def test_errors_and_the_stream_goes_on(cuda):
    _, faces = two_topologies()
    three_on_an_edge = faces.copy()
    three_on_an_edge[1, 7] = [faces[1, 0, 1], faces[1, 0, 0], 85]            # a third face on an edge of face 0
    duplicated = faces.copy()
    duplicated[1, 9] = faces[1, 3]
    for bad in (three_on_an_edge, duplicated):
        with pytest.raises(ValueError, match="batch element 1"):
            mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(bad), 99)        # the host build
        with pytest.raises(ValueError, match="batch element 1"):
            mesh_dihedral.MeshEdgePoints.from_faces(dev_t(bad), 99)
    for value in (99, -1):
        bad = faces.copy()
        bad[1, 17, 1] = value
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(bad), 99)
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_dihedral.MeshEdgePoints.from_faces(dev_t(bad), 99)
        table = np.stack([np.resize(cpu_table(faces[b]), (240, 4)) for b in range(2)])
        table[1, 5, 3] = value
        with pytest.raises(IndexError, match="batch element 1"):
            mesh_dihedral.MeshEdgePoints.from_edge_points(dev_t(table), 99)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), 99)                  # the next call on the stream
    for b in range(2):
        assert_table(topo, b, cpu_table(faces[b]))


# ---------------------------------------------------------------------------------------------- 2. incidence
@pytest.mark.parametrize("name", ["grid_40x130", "fan_300", "fan_8000", "two"])
def test_incidence_lists_are_the_ascending_codes(cuda, name):
    if name == "two":
        faces, n = two_topologies()[1], 99
    else:
        faces, n = named_faces(name)
        faces = faces[None]
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), n)
    start, entries = (t.cpu().numpy() for t in topo.incidence())
    assert start.shape == (faces.shape[0], n + 1) and entries.shape == (faces.shape[0], 4 * topo.capacity)
    for b in range(faces.shape[0]):
        flat = cpu_table(faces[b]).reshape(-1)
        order = np.argsort(flat, kind="stable")            # by vertex, and ascending 4*e + slot within a vertex
        assert np.array_equal(start[b], np.searchsorted(flat[order], np.arange(n + 1)))
        assert np.array_equal(entries[b, :flat.size], order)
    if name == "fan_300":                                  # 301 spokes end at the hub, 300 rim edges have it as both wings
        assert start[0, 1] - start[0, 0] == 901 > 256
    if name == "fan_8000":
        assert start[0, 1] - start[0, 0] == 24001


# ------------------------------------------------------------------------- 3. forward and backward against fp64
@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices (B,N,3) float64 that are exact in fp32, faces (F,3) or (B,F,3), grad_out (B,Ecap) float64)"""
    if name == "cage":
        faces, v = jittered_cage(12, batch=3)
    elif name == "grid_40x130":
        v, faces = folded_grid(40, 130, 13, batch=3)
    elif name == "fan_300":
        v, faces = zigzag_fan(300, 14, batch=3)
    else:
        v, faces = two_topologies()
    v = v.astype(F32).astype(np.float64)
    ecap = 3 * faces.shape[-2]
    g = np.random.default_rng(15).uniform(-1, 1, size=(v.shape[0], ecap)).astype(F32).astype(np.float64)
    return v, faces, g


def tables_of_case(name):
    v, faces, _ = case(name)
    return [cpu_table(faces[b] if faces.ndim == 3 else faces) for b in range(v.shape[0])]


def run(name, device, dtype):
    """(angles (B,Ecap), gradient (B,N,3)) as float64 numpy"""
    v, faces, g = case(name)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(torch.from_numpy(faces).to(device), v.shape[1])
    x = torch.from_numpy(v).to(device=device, dtype=dtype).requires_grad_(True)
    out = mesh_dihedral.mesh_dihedral_angle(x, topo)
    grad, = torch.autograd.grad(out, x, torch.from_numpy(g).to(device=device, dtype=dtype))
    return out.detach().double().cpu().numpy(), grad.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def references(name):
    """the fp64 and the fp32 CPU composition, computed once"""
    return run(name, "cpu", torch.float64), run(name, "cpu", torch.float32)


# The smallest K the fp32 CPU composition meets on the inputs of case(): 0.257 on the cage (0 with another CPU's
# torch build: the larger is kept), 0.0935 on the meshes with boundary edges, whose fp32 clamp bound is not the double's.
K_CPU = {"cage": 0.26, "grid_40x130": 0.094, "fan_300": 0.094, "two_topologies": 0.094}


def forward_ratio(got, ref, d):
    """the largest K for which |got - ref| <= K eps32 / sqrt(1 - d^2) + 4 eps32 pi is tight, over the edges"""
    return float(np.max((np.abs(got - ref) - 4 * EPS32 * np.pi) * np.sqrt(1 - d * d) / EPS32, initial=0.0))


@pytest.mark.parametrize("name", ["cage", "grid_40x130", "fan_300", "two_topologies"])
def test_forward_and_backward_against_the_fp64_composition(cuda, name):
    """Per edge |angle - angle64| <= K eps32 / sqrt(1 - d^2) + 4 eps32 pi with d the fp64 clamped dot, K = 4 x K_CPU,
    the smallest K the fp32 CPU composition was measured to meet on these same inputs (printed again here beside the
    pinned figure); the gradient's error over max |grad64| <= 4 x the same figure of the fp32 CPU composition.
    DESIGN.md "Mesh dihedral angles" records the measured figures."""
    v, faces, _ = case(name)
    tables = tables_of_case(name)
    dots = []
    for b in range(v.shape[0]):
        dots.append(np.clip(assert_clear_of_the_clamp(v[b], tables[b]), LO, HI))      # no edge is left out
    (ref, gref), (c32, g32) = references(name)
    got, ggot = run(name, "cuda", torch.float32)
    assert got.shape == ref.shape and ggot.shape == gref.shape and np.isfinite(got).all() and np.isfinite(ggot).all()
    k_cpu = k_hip = 0.0
    for b in range(v.shape[0]):
        count = tables[b].shape[0]
        k_cpu = max(k_cpu, forward_ratio(c32[b, :count], ref[b, :count], dots[b]))
        k_hip = max(k_hip, forward_ratio(got[b, :count], ref[b, :count], dots[b]))
        assert (got[b, count:] == 0).all() and not np.signbit(got[b, count:]).any()
    bound = 4 * K_CPU[name]
    scale = np.abs(gref).max()
    e_cpu, e_hip = np.abs(g32 - gref).max() / scale, np.abs(ggot - gref).max() / scale
    print("%s: forward K fp32 CPU composition %.3g, HIP %.3g, bound %.3g; gradient error fp32 CPU composition %.3g, "
          "HIP %.3g, bound %.3g" % (name, k_cpu, k_hip, bound, e_cpu, e_hip, 4 * e_cpu))
    assert k_hip <= bound
    assert e_hip <= 4 * e_cpu


# ------------------------------------------------------------------------ 4. fixed values and run-to-run identity
def test_flat_grid_gives_the_two_constants_and_no_gradient(cuda):
    v, faces = grid_mesh(40, 130)
    table = cpu_table(faces)
    boundary = table[:, 2] == table[:, 3]
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), v.shape[0])
    x = dev_t(v[None], True)
    out = mesh_dihedral.mesh_dihedral_angle(x, topo)
    got = out[0, :table.shape[0]].detach().double().cpu().numpy()
    want = np.where(boundary, BOUNDARY, FLAT)
    d = np.where(boundary, LO, HI)
    k = forward_ratio(got, want, d)
    print("flat grid: forward K of HIP %.3g, bound %.3g" % (k, 4 * K_CPU["grid_40x130"]))
    assert k <= 4 * K_CPU["grid_40x130"]          # the same bound as on the folded grid
    grad, = torch.autograd.grad(out.sum(), x)
    assert bool((grad == 0).all())


@contextlib.contextmanager
def deterministic():
    torch.use_deterministic_algorithms(True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(False)


@pytest.mark.parametrize("name", ["fan_300", "two_topologies"])
def test_backward_is_bit_identical_and_ignores_the_padding(cuda, name):
    v, faces, g = case(name)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), v.shape[1])

    def backward(weights):
        x = dev_t(v.astype(F32), True)
        out = mesh_dihedral.mesh_dihedral_angle(x, topo)
        grad, = torch.autograd.grad(out, x, dev_t(weights.astype(F32)))
        return out.detach().cpu().numpy(), grad.cpu().numpy()

    out, first = backward(g)
    assert (first != 0).any()
    for _ in range(2):
        assert backward(g)[1].tobytes() == first.tobytes()
    with deterministic():
        assert backward(g)[1].tobytes() == first.tobytes()
    other = g.copy()
    for b in range(v.shape[0]):
        count = topo.count(b)
        assert count < topo.capacity and (out[b, count:] == 0).all()
        other[b, count:] = np.nan                                     # whatever stands in the padding rows
    assert backward(other)[1].tobytes() == first.tobytes()


# --------------------------------------------------------------------------------------------- 5. the API paths
def test_dihedral_angle_with_an_index_out_of_range(cuda):
    faces, v = jittered_cage(16)
    table = table_of("cage").copy()
    for value in (162, -1, 2 ** 40):
        bad = table.copy()
        bad[7, 3] = value
        x = dev_t(v[0].astype(F32), True)
        out = geo_operations.dihedral_angle(x, dev_t(bad))                  # no exception, no host read
        good = geo_operations.dihedral_angle(dev_t(v[0].astype(F32)), dev_t(table))
        got = out.detach().cpu().numpy()
        assert np.isnan(got[7]) and np.isfinite(np.delete(got, 7)).all()
        assert np.array_equal(np.delete(got, 7), np.delete(good.cpu().numpy(), 7))
        grad, = torch.autograd.grad(out.sum(), x)
        grad = grad.cpu().numpy()
        touched = np.zeros(162, bool)
        touched[bad[7, :3]] = True                                          # the in-range entries of that row
        assert np.isnan(grad[touched]).all() and np.isfinite(grad[~touched]).all()


def test_reference_names_on_cuda_tensors(cuda):
    for name in ("grid_40x130", "cage"):
        faces, n = named_faces(name)
        got = geo_operations.get_edge_points(dev_t(faces))
        assert got.is_cuda and got.dtype == torch.int64
        assert np.array_equal(got.cpu().numpy(), geo_operations.get_edge_points(torch.from_numpy(faces)).numpy())
    # column swaps: the same bits (test_mesh_dihedral_host.py states the rule)
    faces, v = jittered_cage(17)
    table = table_of("cage")
    x = dev_t(v[0].astype(F32))
    base = geo_operations.dihedral_angle(x, dev_t(table))
    some = np.random.default_rng(18).random(table.shape[0]) < 0.5
    for columns in ((0, 1), (2, 3)):
        mixed = np.where(some[:, None], swapped(table, columns), table)
        assert torch.equal(geo_operations.dihedral_angle(x, dev_t(mixed)), base)
        grads = []
        for t in (table, mixed):
            y = dev_t(v[0].astype(F32), True)
            grads.append(torch.autograd.grad(geo_operations.dihedral_angle(y, dev_t(t)).sum(), y)[0])
        # every edge's terms are the same bits either way, and a swap moves a code to the other vertex of its pair,
        # not within a vertex's list (the two codes of a repeated wing carry equal terms): the same sums, bit for bit
        assert torch.equal(grads[0], grads[1])
    normals = geo_operations.get_normals(x, dev_t(table), 0)
    assert normals.shape == (480, 3) and bool(torch.isfinite(normals).all())


# ------------------------------------------------------------------------------- 6. capture and a side stream
def test_step_is_capturable_and_stream_safe(cuda):
    v, faces, g = case("two_topologies")
    other = np.ascontiguousarray(v[::-1]).astype(F32)
    topo = mesh_dihedral.MeshEdgePoints.from_faces(dev_t(faces), 99)           # kept: built outside the capture
    weights = dev_t(g.astype(F32))

    def step(a):
        out = mesh_dihedral.mesh_dihedral_angle(a, topo)
        return (out,) + torch.autograd.grad(out, a, weights)

    x = dev_t(v.astype(F32), True)
    step(x)
    eager = [t.detach().clone() for t in step(dev_t(other, True))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = step(dev_t(other, True))
        step(x)                                                            # and the warm-up of the capture below
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(got, eager):
        assert torch.equal(a.detach(), b)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step(x)
    with torch.no_grad():
        x.copy_(dev_t(other))
    for _ in range(2):
        with torch.no_grad():
            for t in held:
                t.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(held, eager):
            assert torch.equal(a.detach(), b)


# --------------------------------------------------------------------------------------------------- 7. the loss
def run_loss(mode, reduction, device, dtype):
    v, faces, _ = case("two_topologies")
    other = (v + 0.004 * np.random.default_rng(19).uniform(-1, 1, size=v.shape)).astype(F32).astype(np.float64)
    for b in range(2):                                   # the second mesh stays clear of the clamp as well
        assert_clear_of_the_clamp(other[b], cpu_table(faces[b]))
    xs = [torch.from_numpy(a).to(device=device, dtype=dtype).requires_grad_(True) for a in (v, other)]
    mod = model_loss.MeshDihedralAngleLoss(2.4 if mode == "threshold" else None, reduction)
    args = xs if mode == "pair" else xs[:1]
    loss = mod(*args, face=torch.from_numpy(faces).to(device))
    grads = torch.autograd.grad(loss.sum(), args)
    return [loss.detach().double().cpu().numpy()] + [t.double().cpu().numpy() for t in grads]


def measure(got, ref):
    """the largest absolute error over the largest absolute reference"""
    return float(np.abs(got - ref).max(initial=0.0)) / max(float(np.abs(ref).max(initial=0.0)), 1e-30)


@pytest.mark.parametrize("reduction", REDUCTIONS)
@pytest.mark.parametrize("mode", ["pair", "threshold"])
def test_loss_against_the_fp64_composition(cuda, mode, reduction):
    """value and gradients against the fp64 CPU composition; the bound is the standing rule of DESIGN.md "k-NN edge
    operators": 4x the same figure of the fp32 CPU composition, floor 1e-6"""
    ref = run_loss(mode, reduction, "cpu", torch.float64)
    cpu32 = run_loss(mode, reduction, "cpu", torch.float32)
    got = run_loss(mode, reduction, "cuda", torch.float32)
    assert all(np.isfinite(a).all() for a in ref + cpu32 + got)
    for what, g, c, r in zip(("value", "grad vert1", "grad vert2"), got, cpu32, ref):
        err, base = measure(g, r), measure(c, r)
        bound = max(4 * base, 1e-6)
        print("%s %s %s: error %.3g, fp32 CPU composition %.3g, bound %.3g" % (mode, reduction, what, err, base, bound))
        assert g.shape == r.shape and err <= bound, (what, err, bound)


def test_loss_keeps_its_topology(cuda):
    v, faces, _ = case("two_topologies")
    x = dev_t(v.astype(F32))
    mod = model_loss.MeshDihedralAngleLoss(2.4, consistent_topology=True)
    first = mod(x, face=dev_t(faces))
    kept = mod.E
    assert isinstance(kept, mesh_dihedral.MeshEdgePoints) and kept.edge_points.is_cuda
    assert torch.equal(mod(x), first) and mod.E is kept
    fan, n = fan_mesh(8)
    assert mod(dev_t(np.zeros((2, 99, 3), F32)), face=dev_t(fan)) is not None and mod.E is kept   # faces are not looked at
