"""NumPy restatement of the streaming kernels of gnn.cpp_amd/csrc/gnnx_elementwise.hip and of gnnx_sgd_step_f32
(gnnx_train.hip).  The two kinds of reference are those of tests/norm_ref.py: element arithmetic in float32 with one rounding
per operation, compared bit for bit; reductions on inputs whose sum is exact in float32 in any order (`norm_ref.check_exact`:
per output, sum|term| / quantum < 2^24), compared by equality with the float64 sum."""
import numpy as np

from tests.norm_ref import F32, X_VALUES, check_exact, f32

OUT_VALUES = np.array([0.5, -1.75, 3.0, -8.0, 0.25], dtype=np.float32)     # dyadic accumulators for beta * out + sum
BETAS = (0.0, 1.0, 0.5, -2.0)
OUT_QUANTUM = 0.125                                                         # divides beta * out for every beta above


# the shapes of tests/test_gpu_elementwise.py: (F, pad, kernel) on a leading dimension F + pad, and the row counts
COLSUM_WIDTHS = ((4, 0, "vec"), (8, 0, "vec"), (64, 0, "vec"), (256, 0, "vec"), (1024, 0, "vec"), (132, 0, "stage1"), (300, 0, "stage1"),
                 (1028, 0, "stage1"), (256, 1, "stage1"), (1, 0, "narrow"), (7, 0, "narrow"), (33, 0, "narrow"), (100, 0, "narrow"))
COLSUM_ROWS = (0, 1, 63, 65, 127, 129, 70_001)
COLSUM_CASES = [(F, pad, n, k) for F, pad, k in COLSUM_WIDTHS for n in COLSUM_ROWS] + [(4, 0, 400_003, "vec-unrolled")]
SLOT_WIDTHS = (4, 8, 64, 256, 1024)
SLOT_ROWS = (1, 65, 129, 1031)
ROWSUM_COLS = (1, 63, 64, 65, 200, 252, 256, 260, 1024)


def exact_matrix(n, F, seed=0):
    """[n, F] of {-2, -1, 1, 2}: no zeros, so a dropped or doubled row changes every column sum (and a dropped column every row
    sum); sum|x| <= 2 n, exact for n < 2^23."""
    return X_VALUES[np.random.default_rng([seed, n, F]).integers(0, 4, (n, F), dtype=np.uint8)]


def exact_out(F, seed=0):
    return OUT_VALUES[(np.arange(F) + seed) % len(OUT_VALUES)]


def colsum_ref(G, beta=0.0, out=None):
    """out[f] = beta * out[f] + sum_i G[i, f] on exact data.  beta == 0 does not read `out` (it may hold NaN).  The terms of one
    output are the column's entries and beta * out[f]: all multiples of OUT_QUANTUM, asserted exact together."""
    G = f32(G)
    assert np.array_equal(G, np.rint(G)), "the matrix must hold integers"
    acc = np.zeros(G.shape[1]) if beta == 0.0 else np.float64(beta) * f32(out).astype(np.float64)
    quanta = (np.abs(G).sum(0, dtype=np.float64) + np.abs(acc)) / OUT_QUANTUM
    assert np.array_equal(acc / OUT_QUANTUM, np.rint(acc / OUT_QUANTUM)) and quanta.max() < 2.0 ** 24, "colsum input is not exact in every order"
    s = G.sum(0, dtype=np.float64) + acc
    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return s.astype(np.float32)


def colsum_beta_as_flag(G, beta, out):
    """The old behaviour (beta != 0 taken as 1): what the beta = 0.5 and -2 cases must be able to tell from the contract."""
    return colsum_ref(G, 0.0 if beta == 0.0 else 1.0, out)


def rowsum_exact_ref(X):
    X = f32(X)
    check_exact(X.T, 1.0)
    return X.sum(1, dtype=np.float64).astype(np.float32)


def rowsum_ascending_ref(X):
    """out[r] = (((0 + X[r, 0]) + X[r, 1]) + ...) in float32: the documented order for rows of at most 64 columns."""
    X = f32(X)
    acc = np.zeros(X.shape[0], dtype=np.float32)
    for c in range(X.shape[1]):
        acc = acc + X[:, c]
    return acc


def axpy_ref(a, x, y):
    """y + a * x: the product rounded, then the sum."""
    return f32(f32(y) + F32(a) * f32(x))


def sgd_ref(p, g, lr, wd):
    """p - lr * (g + wd * p); the `+ wd * p` is skipped when wd == 0 (so g = -0 keeps its sign and an infinite p makes no NaN)."""
    p, g = f32(p), f32(g)
    with np.errstate(all="ignore"):
        if wd != 0.0:
            g = g + F32(wd) * p
        return f32(p - F32(lr) * g)


def gather_ref(X, idx):
    return f32(X)[np.asarray(idx, dtype=np.int64)]


def scatter_add_ref(Y, inp, idx):
    """Y[idx[k], :] += inp[k, :] for UNIQUE idx (the kernel has no atomics: a repeated index within one call is a race)."""
    idx = np.asarray(idx, dtype=np.int64)
    assert len(np.unique(idx)) == len(idx), "scatter_add_rows needs unique indices within one call"
    out = f32(Y).copy()
    out[idx] = out[idx] + f32(inp)
    return out


def slot_table_ref(send_idx, n_rows, slots_per_row=8):
    """[n_rows, 8] int32: row r's positions in the send list, ascending, packed to the front, -1 behind."""
    table = np.full((n_rows, slots_per_row), -1, dtype=np.int32)
    fill = np.zeros(n_rows, dtype=np.int64)
    for slot, r in enumerate(np.asarray(send_idx, dtype=np.int64)):
        assert fill[r] < slots_per_row - 1, "a row goes to at most 7 slots"
        table[r, fill[r]] = slot
        fill[r] += 1
    return table


def rows_to_slots_ref(X, table, n_slots, sentinel):
    """send[slot, :] = X[row, :] for every slot listed in the table; the other rows of `send` keep the sentinel."""
    X = f32(X)
    send = np.full((n_slots, X.shape[1]), sentinel, dtype=np.float32)
    for r in range(table.shape[0]):
        for s in table[r]:
            if s < 0:
                break
            send[s] = X[r]
    return send


def send_list(n_rows, per_row, seed=0):
    """A send list in which row r appears per_row[r % len(per_row)] times, in shuffled slot order."""
    rows = np.concatenate([np.full(per_row[r % len(per_row)], r, dtype=np.int32) for r in range(n_rows)] + [np.zeros(0, dtype=np.int32)])
    return np.random.default_rng([seed, n_rows]).permutation(rows).astype(np.int32)


# bfloat16 special values: (float32 bits, what).  Expected results come from torch.bfloat16 in the tests and from the plain
# round-to-nearest-even below in the CPU test.
BF16_TABLE = np.array([
    0x3F808000,   # 1 + 2^-8: tie, even below -> rounds DOWN to 0x3F80
    0x3F818000,   # tie, odd below -> rounds UP to 0x3F82
    0x3F808001,   # just above a tie -> up
    0x3F807FFF,   # just below a tie -> down
    0xBF808000, 0xBF818000,             # the same ties, negative
    0x7F7FFFFF, 0xFF7FFFFF,             # largest finite -> +-inf
    0x7F7F7FFF,                         # below the last tie -> stays finite (0x7F7F)
    0x7F7F8000,                         # the last tie: odd below -> up to inf
    0x7F800000, 0xFF800000,             # +-inf
    0x00000000, 0x80000000,             # +-0
    0x00000001, 0x80000001,             # smallest denormals -> +-0
    0x00008000, 0x00018000,             # denormal ties: to even (0x0000), to even (0x0002)
    0x007FFFFF,                         # largest denormal -> smallest normal 0x0080
    0x00800000,                         # smallest normal
    0x3F800000, 0xC0490FDB,             # 1, -pi
], dtype=np.uint32)
BF16_NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FBFFFFF, 0xFF80FFFF], dtype=np.uint32)


def bf16_rne_ref(u32):
    """Round-to-nearest-even of float32 bit patterns to bfloat16 bit patterns (finite and infinite inputs)."""
    u = np.asarray(u32, dtype=np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
