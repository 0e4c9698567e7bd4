"""What the mesh operators (mesh_edges, mesh_dihedral, mesh_laplacian) share: the contract of a topology object, kept
true in one place.

    index_table     a caller's integer tensor -> the contiguous int64 (Bt, rows, cols) table; an un-batched tensor or
                    a view with batch stride 0 is ONE topology that a whole batch shares (Bt == 1)
    out_of_range    the CPU range check, one flag per batch element
    raise_flagged   IndexError / ValueError naming the first flagged batch element
    VertexTable     a counted row table (Bt, Ecap, cols) over n_vertices vertices with its lazy vertex lists: the base
                    of MeshEdges (cols = 2) and MeshEdgePoints (cols = 4)
    check_vertices  a step's argument checks
    gather_function the autograd Function of a step: forward over the table, backward a gather over the vertex lists

A topology is built once, with EXACTLY ONE device-to-host copy (counts and flags together), and nothing that uses it
afterwards synchronises with the host; an index outside ``[0, n_vertices)`` raises IndexError naming the batch element
when it is built and gives NaN in a step on a table that was never checked.  DESIGN.md "Mesh edge operators" states
the contract and how a new mesh operator plugs in.
"""
import ctypes

import torch

from . import _lib

LIMIT = 2 ** 31 - 1   # csrc/mesh_edges.hip: the index words in use


def is_index(t):
    return not (t.is_floating_point() or t.is_complex() or t.dtype == torch.bool)


def workspace(dev, bt, n, items):
    """``(pointer, byte count, tensor)`` of the list builds' scratch; the caller holds the tensor across its launch"""
    nbytes = int(_lib.lib().pp_mesh_edges_workspace_bytes(bt, n, items))
    ws = _lib.workspace(dev, "mesh_edges", nbytes)
    return (_lib.ptr(ws) if ws is not None else None), ctypes.c_size_t(nbytes), ws


def fits(what, bt, n, items):
    if bt * items > LIMIT or bt * (n + 1) > LIMIT:
        raise NotImplementedError("%s: %d batch elements of %d entries over %d vertices do not fit the kernels' 32-bit "
                                  "index words" % (what, bt, items, n))


def index_table(what, name, t, shape, cols_ok, keep=None, triangles=None):
    """The argument ``name`` of ``what``, an integer tensor (rows, cols) or (B, rows, cols) with ``cols_ok(cols)``, as
    contiguous int64 ``(Bt, rows, cols[:keep])``.  ``shape`` is the shape as the ValueError spells it; with
    ``triangles`` (the words after "triangles only") a column count other than 3 is NotImplementedError instead."""
    if not isinstance(t, torch.Tensor) or not is_index(t):
        raise TypeError("%s: %s must be an integer tensor, got %s"
                        % (what, name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or (triangles is None and not cols_ok(t.shape[-1])):
        raise ValueError("%s: %s must have shape %s, got %s" % (what, name, shape, tuple(t.shape)))
    if triangles is not None and t.shape[-1] != 3:
        raise NotImplementedError("%s: triangles only%s, got faces of %d corners" % (what, triangles, t.shape[-1]))
    if t.shape[0] > 1 and t.stride(0) == 0:
        t = t[:1]
    if keep is not None:
        t = t[..., :keep]
    return (t if t.dtype == torch.int64 else t.long()).contiguous()


def out_of_range(table, n_vertices):
    """CPU ``table`` (Bt, ...) -> per batch element, whether it holds an index outside [0, n_vertices)"""
    return ((table < 0) | (table >= n_vertices)).reshape(table.shape[0], -1).any(1).tolist()


def raise_flagged(what, range_flags, manifold_flags=()):
    for b, flag in enumerate(range_flags):
        if flag:
            raise IndexError("%s: batch element %d holds a vertex index outside [0, n_vertices)" % (what, b))
    for b, flag in enumerate(manifold_flags):
        if flag:
            raise ValueError("%s: batch element %d has an edge with more than two incident half-edges (a "
                             "non-manifold edge or a duplicated face)" % (what, b))


_INCIDENCE = {2: ("pp_mesh_edge_incidence", "edge incidence"),
              4: ("pp_mesh_edge_points_incidence", "edge-points incidence")}


def incidence_hip(rows, counts, n_vertices, flags):
    """contiguous int64 CUDA ``rows`` (Bt,Ecap,cols), cols 2 or 4, int32 ``counts`` (Bt) -> ``(start (Bt,N+1) int32,
    entries (Bt,cols*Ecap) as int32 storage)``: vertex v's slice holds ``cols*e + column`` of its entries in the rows
    ``e < counts[b]``, ascending; an entry out of range is ORed into ``flags`` (Bt, initialised)."""
    dev = rows.device
    bt, ecap, cols = rows.shape
    entry, label = _INCIDENCE[cols]
    fits(label, bt, n_vertices, cols * ecap)
    start = torch.empty(bt, n_vertices + 1, dtype=torch.int32, device=dev)
    entries = torch.empty(bt, cols * ecap, dtype=torch.int32, device=dev)
    with _lib.on_device(dev) as stream:
        wsp, nbytes, ws = workspace(dev, bt, n_vertices, cols * ecap)
        _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(rows), _lib.ptr(counts), _lib.ptr(start), _lib.ptr(entries),
                                              _lib.ptr(flags), bt, ecap, n_vertices, wsp, nbytes, stream),
                   "mesh " + label)
    return start, entries


class VertexTable(object):
    """A batch of row tables over ``n_vertices`` vertices each: ``_rows`` (Bt,Ecap,COLS) int64, rows ``[0, count[b])``
    in use and later rows -1; ``counts`` (Bt,) int32 on the device; ``counts_host`` the same numbers as a tuple of
    Python ints; ``incidence()`` the vertex lists the backward gathers over (CUDA only).  A subclass names its columns
    (``COLS``, ``NAME``), aliases ``_rows`` under its public spelling and adds its constructors."""

    COLS = None
    NAME = None   # the table in messages

    def __init__(self, rows, counts, counts_host, n_vertices, incidence=None):
        self._rows = rows
        self.counts = counts
        self.counts_host = counts_host
        self.n_vertices = int(n_vertices)
        self._incidence = incidence

    @property
    def batch(self):
        return self._rows.shape[0]

    @property
    def capacity(self):
        return self._rows.shape[1]

    def count(self, b):
        """the number of edges of batch element ``b`` of the vertices (a Python int)"""
        return self.counts_host[0 if self.batch == 1 else b]

    def _view(self, b):
        return self._rows[0 if self.batch == 1 else b, :self.count(b)]

    def incidence(self):
        """``(start, entries)``; built here, without a host read, for an object made by ``_unchecked``"""
        if self._incidence is None:
            flags = torch.zeros(self.batch, dtype=torch.int32, device=self._rows.device)
            self._incidence = incidence_hip(self._rows, self.counts, self.n_vertices, flags)
        return self._incidence

    @classmethod
    def _unchecked(cls, rows, n_vertices):
        """int64 ``rows`` (Bt,E,COLS), every row in use, nothing read back: the incidence is built on first use and an
        out-of-range index is not reported (the step kernels give NaN for it)."""
        bt, e = rows.shape[0], rows.shape[1]
        counts = torch.full((bt,), e, dtype=torch.int32, device=rows.device)
        return cls(rows, counts, (e,) * bt, n_vertices)

    @classmethod
    def _padded(cls, lists, like, capacity, n_vertices):
        """CPU: the row lists of the batch elements -> the object over their (Bt,capacity,COLS) table"""
        rows = like.new_full((len(lists), capacity, cls.COLS), -1)
        for b, part in enumerate(lists):
            rows[b, :part.shape[0]] = part
        host = tuple(int(part.shape[0]) for part in lists)
        return cls(rows, torch.tensor(host, dtype=torch.int32), host, n_vertices)

    @classmethod
    def _read_back(cls, what, rows, status, n_vertices):
        """CUDA ``rows`` with their counts in ``status[0]``; builds the vertex lists (range flags into ``status[1]``)
        and reads ``status`` (int32 (2 or 3, Bt): counts, range flags, manifold flags) back: the one copy"""
        incidence = incidence_hip(rows, status[0], n_vertices, status[1])
        host = status.tolist()
        raise_flagged(what, *host[1:])
        return cls(rows, status[0], tuple(host[0]), n_vertices, incidence)

    @classmethod
    def _from_rows(cls, what, rows, n_vertices):
        """a caller's normalised table, every row in use"""
        bt, e = rows.shape[0], rows.shape[1]
        if not rows.is_cuda:
            raise_flagged(what, out_of_range(rows, n_vertices))
            return cls(rows, torch.full((bt,), e, dtype=torch.int32), (e,) * bt, n_vertices)
        status = torch.empty(2, bt, dtype=torch.int32, device=rows.device)
        status[0] = e
        status[1] = 0
        return cls._read_back(what, rows, status, n_vertices)


def check_vertices(what, vertices, topo, kind, name="topo", rows="_rows", d3=False):
    """``vertices`` (B,N,D), D = 3 with ``d3``, against the topology ``topo``: argument ``name``, of class ``kind``,
    its tensor the attribute ``rows``"""
    if not isinstance(topo, kind):
        raise TypeError("%s: %s must be a %s, got %s" % (what, name, kind.__name__, type(topo).__name__))
    if vertices.dim() != 3 or (d3 and vertices.shape[2] != 3):
        raise ValueError("%s: vertices must have shape (B, N, %s), got %s"
                         % (what, "3" if d3 else "D", tuple(vertices.shape)))
    if not vertices.is_floating_point():
        raise RuntimeError("%s: vertices must be a floating tensor, got %s" % (what, vertices.dtype))
    if vertices.shape[1] != topo.n_vertices:
        raise ValueError("%s: the topology was built for %d vertices, got %d"
                         % (what, topo.n_vertices, vertices.shape[1]))
    if topo.batch not in (1, vertices.shape[0]):
        raise ValueError("%s: a topology of %d batch elements does not serve %d vertex sets"
                         % (what, topo.batch, vertices.shape[0]))
    device = getattr(topo, rows).device
    if device != vertices.device:
        raise RuntimeError("%s: the topology is on %s, expected %s" % (what, device, vertices.device))


def gather_function(name, doc, forward_entry, backward_entry, what):
    """The autograd Function ``name`` of a step ``what`` on a ``VertexTable``: ``forward_entry(vertices, rows, counts,
    out (B,Ecap), ...)``, one value per row, and ``backward_entry(vertices, rows, start, entries, grad_out, grad,
    ...)``, a gather over the vertex lists (CUDA fp32)."""
    forward_what, backward_what = what + " forward", what + " backward"

    def forward(ctx, vertices, topo):
        dev = _lib.require_cuda(("vertices", vertices), (topo.NAME, topo._rows))
        vertices = vertices.contiguous()
        b, n, _ = vertices.shape
        ecap = topo.capacity
        out = torch.empty(b, ecap, dtype=torch.float32, device=dev)
        with _lib.on_device(dev) as stream:
            _lib.check(getattr(_lib.lib(), forward_entry)(
                _lib.ptr(vertices), _lib.ptr(topo._rows), _lib.ptr(topo.counts), _lib.ptr(out), b, n, ecap,
                int(topo.batch == 1), stream), forward_what)
        ctx.save_for_backward(vertices)
        ctx.topo = topo
        return out

    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None
        (vertices,) = ctx.saved_tensors
        topo = ctx.topo
        dev = vertices.device
        b, n, _ = vertices.shape
        grad_out = grad_out.contiguous()
        grad = torch.empty_like(vertices)
        with _lib.on_device(dev):
            start, entries = topo.incidence()
        with _lib.on_device(dev) as stream:
            _lib.check(getattr(_lib.lib(), backward_entry)(
                _lib.ptr(vertices), _lib.ptr(topo._rows), _lib.ptr(start), _lib.ptr(entries), _lib.ptr(grad_out),
                _lib.ptr(grad), b, n, topo.capacity, int(topo.batch == 1), stream), backward_what)
        return grad, None

    return type(torch.autograd.Function)(name, (torch.autograd.Function,), {
        "__doc__": doc, "forward": staticmethod(forward), "backward": staticmethod(backward)})
