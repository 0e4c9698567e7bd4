"""CPU test (no GPU) of the workspace that ball_query, three_nn and knn_points share (csrc/grid_pairs.h): a reference
cloud counting-sorted into the uniform grid and a query cloud in Morton order.  The sizes are pure host arithmetic; the
expected values restate the layout here, so that a change of the layout has to be made twice to pass."""
from pytorch_points_amd import _lib

GRID_CELLS = 32768          # pp::kGridCells (grid_common.h): 32 cells per axis


def align256(x):
    return (x + 255) // 256 * 256


def pair_bytes(b, n_ref, n_query):
    """2B grid sets of 64 bytes, B tables of kGridCells + 1 cell starts, the sorted reference cloud and the sorted
    queries as 16-byte records; every region but the last rounded up to 256 bytes"""
    return align256(128 * b) + align256(4 * (GRID_CELLS + 1) * b) + align256(16 * b * n_ref) + 16 * b * n_query


def test_the_restatement_itself():
    assert pair_bytes(1, 1024, 1024) == 256 + 131328 + 16384 + 16384
    assert pair_bytes(3, 1025, 1039) == 512 + 393472 + 49408 + 49872


# n_ref and n_query on both sides of a multiple of 16 (16 * n_ref of a multiple of 256), B = 1 and B = 3
SHAPES = [(b, r, q) for b in (1, 3) for r, q in [(4096, 4096), (4111, 4097), (4097, 4111), (5000, 4111),
                                                  (4112, 4113), (8191, 8193)]]


def test_three_nn_workspace_bytes_follow_the_layout():
    size = _lib.lib().pp_three_nn_workspace_bytes            # (B, N unknown = queries, M known = reference)
    for b, r, q in SHAPES + [(1, 1024, 1024), (3, 1024, 1025), (3, 1025, 1024), (1, 1039, 1041), (1, 1024, 2 ** 31 - 1)]:
        assert size(b, q, r) == pair_bytes(b, r, q), (b, r, q)
    for b, n, m in [(0, 4096, 4096), (-1, 4096, 4096), (1, 1023, 1024), (1, 1024, 1023), (3, 1023, 4096),
                    (2, 1 << 30, 1024), (2, 1024, 1 << 30), (3, 1 << 30, 1 << 30)]:
        assert size(b, n, m) == 0, (b, n, m)


def test_knn_workspace_bytes_follow_the_layout():
    size = _lib.lib().pp_knn_workspace_bytes                 # (B, N of p1 = queries, M of p2 = reference, K)
    for k in (1, 8, 32):
        for b, r, q in SHAPES + [(1, 1024, 1024), (3, 1024, 1025), (3, 1025, 1024), (1, 1039, 1041),
                                 (1, 1024, 2 ** 31 - 1)]:
            assert size(b, q, r, k) == pair_bytes(b, r, q), (b, r, q, k)
    for b, n, m, k in [(0, 4096, 4096, 8), (1, 1023, 1024, 8), (1, 1024, 1023, 8), (1, 4096, 4096, 0),
                       (1, 4096, 4096, 33), (1, 4096, 127, 32), (1, 4096, 100, 32),      # M < 4K (and below 1024)
                       (2, 1 << 30, 1024, 8), (2, 1024, 1 << 30, 8)]:
        assert size(b, n, m, k) == 0, (b, n, m, k)


def test_ball_query_workspace_bytes_follow_the_layout():
    size = _lib.lib().pp_ball_query_workspace_bytes          # (B, N of xyz = reference, M centres = queries, nsample)
    for nsample in (1, 64):
        for b, r, q in SHAPES + [(1, 4096, 1), (3, 4096, 17), (1, 4097, 1023), (3, 524288, 1024), (1, 4096, 2 ** 31 - 1)]:
            assert size(b, r, q, nsample) == pair_bytes(b, r, q), (b, r, q, nsample)
    for b, n, m, nsample in [(0, 4096, 1024, 64), (1, 4095, 1024, 64), (3, 4095, 4096, 64), (1, 4096, 0, 64),
                             (1, 4096, 1024, 0), (1, 524289, 1024, 64),
                             (1, 4096, 1024, 1 << 20),                                   # a wave's rows exceed the LDS
                             (8192, 1 << 18, 1024, 64), (2, 4096, 1 << 30, 64)]:
        assert size(b, n, m, nsample) == 0, (b, n, m, nsample)
