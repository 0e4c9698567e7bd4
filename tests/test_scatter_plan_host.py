"""CPU tests (no GPU) of the one dispatch policy of the scatter-add backwards -- gather_backward, group_points_grad,
three_interpolate_grad, fp32 and 16-bit (sampling.hip: scatter_plan) -- through the plan query of
include/pp_hip_debug.h.

The table states, row by row, the form the dispatch code had written out per entry point before it became one
function: each boundary at the smallest shape on either side of the flip.  A row is (operator, (B, C, sources,
destinations), workspace, (group_points_grad variant, three_interpolate_grad variant, scatter mode)) ->
(fp32 form, 16-bit form, ordered form).  sources / destinations per batch element: M / N of gather_backward,
npoint * nsample / N of group_points_grad, N / M of three_interpolate_grad.  Workspace: "full" = what
pp_scatter_workspace_bytes asks for (0 where the sorted forms do not apply: more than 20480 destinations), "short" =
one byte less, "none".  A 16-bit or ordered NONE is the entry point's PP_ENOTSUP (include/pp_hip.h)."""
import ctypes

import pytest

from pytorch_points_amd import _lib

GATHER, GROUP, INTERP = 0, 1, 2
NONE, ATOMICS, COLUMN, SORTED, ORDERED = 0, 1, 2, 3, 4
K0 = (0, 0, 0)

TABLE = [
    # ---- group_points_grad: the column's floor of 4096 positions; without a workspace fp32 has its atomics, 16-bit nothing
    (GROUP, (1, 1, 4095, 100), "none", K0, (ATOMICS, NONE, NONE)),
    (GROUP, (1, 1, 4096, 100), "none", K0, (COLUMN, COLUMN, NONE)),
    (GROUP, (1, 1, 4095, 100), "full", K0, (ATOMICS, SORTED, ORDERED)),     # (too small for fp32 to sort)
    (GROUP, (1, 1, 4096, 100), "full", K0, (COLUMN, COLUMN, ORDERED)),
    # short lists (P <= 4 N) of a big problem (B P C >= 2^20) are sorted: P at 4 N and 4 N + 4 ...
    (GROUP, (8, 8, 16384, 4096), "full", K0, (SORTED, SORTED, ORDERED)),
    (GROUP, (8, 8, 16388, 4096), "full", K0, (COLUMN, COLUMN, ORDERED)),
    # ... and B P C just under 2^20 (63 * 16384) and at it
    (GROUP, (1, 63, 16384, 4096), "full", K0, (COLUMN, COLUMN, ORDERED)),
    (GROUP, (1, 64, 16384, 4096), "full", K0, (SORTED, SORTED, ORDERED)),
    # the sorted forms end at 20480 destinations
    (GROUP, (1, 64, 16384, 20480), "full", K0, (SORTED, SORTED, ORDERED)),
    (GROUP, (1, 64, 16384, 20481), "full", K0, (COLUMN, COLUMN, NONE)),
    (GROUP, (2, 3, 64, 20480), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (GROUP, (2, 3, 64, 20481), "full", K0, (ATOMICS, NONE, NONE)),
    # the column splits into at most 16 ranges of 19456 destinations
    (GROUP, (1, 1, 4096, 311296), "none", K0, (COLUMN, COLUMN, NONE)),
    (GROUP, (1, 1, 4096, 311297), "none", K0, (ATOMICS, NONE, NONE)),
    # a workspace one byte short is no workspace
    (GROUP, (1, 64, 16384, 4096), "short", K0, (COLUMN, COLUMN, NONE)),
    (GROUP, (2, 3, 64, 100), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (GROUP, (2, 3, 64, 100), "short", K0, (ATOMICS, NONE, NONE)),
    # variant 1: no column (the sorted form keeps its place)
    (GROUP, (1, 1, 4096, 100), "none", (1, 0, 0), (ATOMICS, NONE, NONE)),
    (GROUP, (1, 1, 4096, 100), "full", (1, 0, 0), (ATOMICS, SORTED, ORDERED)),
    (GROUP, (1, 64, 16384, 4096), "full", (1, 0, 0), (SORTED, SORTED, ORDERED)),
    # variant 2: the column below 4096 positions as well -- not beyond 16 ranges, and not in front of the sorted form
    # (the fp32 entries' reading, now the one meaning: the 16-bit template used to put the column first here)
    (GROUP, (2, 3, 64, 100), "none", (2, 0, 0), (COLUMN, COLUMN, NONE)),
    (GROUP, (2, 3, 64, 100), "full", (2, 0, 0), (COLUMN, COLUMN, ORDERED)),
    (GROUP, (1, 1, 64, 311297), "none", (2, 0, 0), (ATOMICS, NONE, NONE)),
    (GROUP, (1, 64, 16384, 4096), "full", (2, 0, 0), (SORTED, SORTED, ORDERED)),
    # scatter mode 1: never sorted; the ordered form is not a choice
    (GROUP, (1, 64, 16384, 4096), "full", (0, 0, 1), (COLUMN, COLUMN, ORDERED)),
    (GROUP, (2, 3, 64, 100), "full", (0, 0, 1), (ATOMICS, NONE, ORDERED)),

    # ---- three_interpolate_grad: the column from 2048 points ...
    (INTERP, (1, 1, 2047, 100), "none", K0, (ATOMICS, NONE, NONE)),
    (INTERP, (1, 1, 2048, 100), "none", K0, (COLUMN, COLUMN, NONE)),
    (INTERP, (1, 1, 2047, 100), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (INTERP, (1, 1, 2048, 100), "full", K0, (COLUMN, COLUMN, ORDERED)),
    # ... while it fits 152 KiB: M at 19456 and 19457
    (INTERP, (1, 1, 2048, 19456), "none", K0, (COLUMN, COLUMN, NONE)),
    (INTERP, (1, 1, 2048, 19457), "none", K0, (ATOMICS, NONE, NONE)),
    (INTERP, (1, 1, 2048, 19457), "full", K0, (ATOMICS, SORTED, ORDERED)),
    # the sorted forms end at M = 20480
    (INTERP, (1, 1, 2048, 20480), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (INTERP, (1, 1, 2048, 20481), "full", K0, (ATOMICS, NONE, NONE)),
    (INTERP, (1, 64, 5462, 20481), "full", K0, (ATOMICS, NONE, NONE)),
    # fp32 sorts from B 3N C = 2^20: 3 * 5461 * 64 = 2^20 - 64, 3 * 5462 * 64 = 2^20 + 128
    (INTERP, (1, 64, 5461, 20480), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (INTERP, (1, 64, 5462, 20480), "full", K0, (SORTED, SORTED, ORDERED)),
    (INTERP, (1, 64, 5462, 20480), "short", K0, (ATOMICS, NONE, NONE)),
    (INTERP, (1, 64, 5462, 100), "full", K0, (COLUMN, COLUMN, ORDERED)),       # (the column comes first)
    # variants 1 and 3: no column
    (INTERP, (1, 1, 2048, 100), "none", (0, 1, 0), (ATOMICS, NONE, NONE)),
    (INTERP, (1, 1, 2048, 100), "full", (0, 1, 0), (ATOMICS, SORTED, ORDERED)),
    (INTERP, (1, 1, 2048, 100), "full", (0, 3, 0), (ATOMICS, SORTED, ORDERED)),
    (INTERP, (1, 64, 5462, 100), "full", (0, 1, 0), (SORTED, SORTED, ORDERED)),
    (INTERP, (1, 64, 5462, 100), "full", (0, 3, 0), (SORTED, SORTED, ORDERED)),
    # variant 2: the column below 2048 points as well -- where it fits
    (INTERP, (1, 1, 2047, 100), "none", (0, 2, 0), (COLUMN, COLUMN, NONE)),
    (INTERP, (1, 1, 7, 19456), "full", (0, 2, 0), (COLUMN, COLUMN, ORDERED)),
    (INTERP, (1, 1, 7, 19457), "none", (0, 2, 0), (ATOMICS, NONE, NONE)),
    # scatter mode 1
    (INTERP, (1, 64, 5462, 20480), "full", (0, 0, 1), (ATOMICS, NONE, ORDERED)),

    # ---- gather_backward: fp32 sorts from B M C = 2^20, 16-bit whenever it can
    (GATHER, (1, 63, 16384, 100), "full", K0, (ATOMICS, SORTED, ORDERED)),
    (GATHER, (1, 64, 16384, 100), "full", K0, (SORTED, SORTED, ORDERED)),
    (GATHER, (1, 64, 16384, 100), "none", K0, (ATOMICS, NONE, NONE)),
    (GATHER, (1, 64, 16384, 100), "short", K0, (ATOMICS, NONE, NONE)),
    (GATHER, (1, 64, 16384, 20480), "full", K0, (SORTED, SORTED, ORDERED)),
    (GATHER, (1, 64, 16384, 20481), "full", K0, (ATOMICS, NONE, NONE)),
    (GATHER, (1, 64, 16384, 100), "full", (0, 0, 1), (ATOMICS, NONE, ORDERED)),
    # the other operators' knobs do not reach it
    (GATHER, (1, 64, 16384, 100), "full", (1, 1, 0), (SORTED, SORTED, ORDERED)),
]

KNOBS = ["group_points_grad_variant", "three_interpolate_grad_variant", "scatter_mode"]


def set_knobs(values):
    for name, v in zip(KNOBS, values):
        fn = getattr(_lib.lib(), "pp_debug_set_" + name)
        fn.argtypes = [ctypes.c_int]
        fn.restype = None
        fn(v)


def plan(op, elem_bytes, write, ordered, shape, ws_bytes):
    fn = _lib.lib().pp_debug_scatter_plan
    fn.argtypes = [ctypes.c_int] * 6 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_size_t]
    fn.restype = ctypes.c_int
    b, c, sources, destinations = shape
    return fn(op, elem_bytes, write, ordered, b, c, sources, destinations, ws_bytes)


def workspace_bytes(op, shape, kind):
    b, _, sources, destinations = shape
    per_source = 3 if op == INTERP else 1
    need = int(_lib.lib().pp_scatter_workspace_bytes(b, per_source * sources, destinations, per_source,
                                                     1 if op == INTERP else 0))
    assert (need == 0) == (destinations > 20480), "the table's shapes stay within the sort's chunk limits"
    return {"full": need, "short": max(need - 1, 0), "none": 0}[kind]


def row_id(row):
    op, shape, ws, knobs, _ = row
    return "%s-%s-%s-k%s" % (["gather", "group", "interp"][op], "x".join(map(str, shape)), ws, "".join(map(str, knobs)))


def entry_code(op, suffix, shape, ws_bytes, ordered):
    """the entry point itself on dummy non-null pointers: PP_ENOTSUP is decided before anything is dereferenced or any
    device looked at (call it ONLY where the plan is NONE)"""
    L = _lib.lib()
    b, c, sources, destinations = shape
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = p if ws_bytes else None
    tail = (ws, ws_bytes) + ((ordered,) if suffix != "f32" else ()) + (None,)
    kind = "out_ws" if suffix != "f32" else "ordered"
    if op == GATHER:
        return getattr(L, "pp_gather_backward_%s_%s" % (kind, suffix))(p, p, p, b, c, destinations, sources, *tail)
    if op == GROUP:
        return getattr(L, "pp_group_points_grad_%s_%s" % (kind, suffix))(p, p, p, b, c, destinations, sources, 1,
                                                                         c * sources, *tail)
    return getattr(L, "pp_three_interpolate_grad_%s_%s" % (kind, suffix))(p, p, p, p, b, c, sources, destinations, *tail)


@pytest.mark.parametrize("row", TABLE, ids=row_id)
def test_plan_table(row):
    op, shape, ws_kind, knobs, (f32, b16, ordered) = row
    ws = workspace_bytes(op, shape, ws_kind)
    set_knobs(knobs)
    try:
        assert plan(op, 4, 0, 0, shape, ws) == f32                      # fp32, accumulating (_f32 with ws 0, _ws_f32)
        if op == GROUP:
            assert plan(op, 4, 1, 0, shape, ws) == f32                  # fp32, written (_out_ws_f32): the same rule
        assert plan(op, 2, 1, 0, shape, ws) == b16                      # f16 / bf16
        assert plan(op, 4, 0, 1, shape, ws) == ordered                  # *_ordered_f32
        assert plan(op, 2, 1, 1, shape, ws) == ordered                  # the 16-bit entries' flag
        # ... and the entry points answer PP_ENOTSUP exactly there
        for suffix in ("f16", "bf16"):
            if b16 == NONE:
                assert entry_code(op, suffix, shape, ws, 0) == _lib.PP_ENOTSUP
            if ordered == NONE:
                assert entry_code(op, suffix, shape, ws, 1) == _lib.PP_ENOTSUP
        if ordered == NONE:
            assert entry_code(op, "f32", shape, ws, 1) == _lib.PP_ENOTSUP
    finally:
        set_knobs(K0)


def test_table_covers_every_form_of_every_operator():
    seen = {(op, col, forms[col]) for op, _, _, _, forms in TABLE for col in range(3)}
    for op in (GATHER, GROUP, INTERP):
        columns = () if op == GATHER else (COLUMN,)
        for form in (ATOMICS, SORTED) + columns:
            assert (op, 0, form) in seen
        for form in (NONE, SORTED) + columns:
            assert (op, 1, form) in seen
        assert (op, 2, ORDERED) in seen and (op, 2, NONE) in seen
        assert (op, 1, ATOMICS) not in seen                              # no 16-bit floating-point atomics


def test_plan_query_is_host_only_and_rejects_what_describes_no_call():
    """pure host arithmetic, like the *_workspace_bytes queries: there is no GPU here.  The entries serve empty and
    negative sizes before any form is chosen, so the query has no answer for them."""
    assert plan(GROUP, 4, 0, 0, (32, 64, 4096 * 64, 16384), 0) == COLUMN    # (config 4 of the benchmark)
    for shape in ((0, 4, 8, 8), (2, 0, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0), (-1, 4, 8, 8), (2, 4, 1 << 31, 8)):
        assert plan(GATHER, 4, 0, 0, shape, 0) == -1
    assert plan(3, 4, 0, 0, (2, 4, 8, 8), 0) == -1 and plan(-1, 4, 0, 0, (2, 4, 8, 8), 0) == -1
    assert plan(GATHER, 8, 0, 0, (2, 4, 8, 8), 0) == -1 and plan(GATHER, 1, 0, 0, (2, 4, 8, 8), 0) == -1
