"""NumPy restatement of the fused graph-attention calls (include/gnnx.h "fused graph attention").  t, e, the row maximum and the
argument e - m are float32 -- single exactly rounded operations, so rowmax must compare equal -- everything from exp on is float64.
Each function also returns S, the float64 sum of the absolute terms of every output element, for the derived bars
    |got - ref| <= c * 2^-24 * S
whose c (rounded operations on the longest chain, + 4 for expf) the functions at the bottom restate from the header's ORDER."""
import numpy as np

from tests.edge_softmax_ref import row_of_entries

SEG = 4096


def segsum(v, keys, n):
    """float64 [n, ...]: the sums of the rows of v by key (rows without a key: 0)."""
    order = np.argsort(keys, kind="stable")
    ptr = np.searchsorted(keys[order], np.arange(n + 1))
    out = np.zeros((n,) + v.shape[1:], dtype=np.float64)
    some = ptr[1:] > ptr[:-1]
    if len(order):
        out[some] = np.add.reduceat(v[order], ptr[:-1][some], axis=0)
    return out


def scores(rowptr, colidx, rowterm, colterm, slope):
    """(t float32 [nnz, H], e - m float32, m float32 [n_rows, H]): the part both sides compute bit for bit."""
    rows = row_of_entries(rowptr)
    t = rowterm[rows] + colterm[colidx]
    e = np.where(t > 0, t, t * np.float32(slope)).astype(np.float32)
    m = np.full((len(rowptr) - 1, t.shape[1]), -np.inf, dtype=np.float32)
    np.maximum.at(m, rows, e)
    return t, (e - m[rows]).astype(np.float32), m


def forward(rowptr, colidx, X, H, rowterm, colterm, slope, bias, relu):
    """dict(Y, rowmax, rowsum, alpha, S_Y): Y float64 [n_rows, F], alpha float64 [nnz, H]."""
    rows, n = row_of_entries(rowptr), len(rowptr) - 1
    D = X.shape[1] // H
    _, arg, m = scores(rowptr, colidx, rowterm, colterm, slope)
    x = np.exp(arg.astype(np.float64))
    z = segsum(x, rows, n)
    alpha = x / z[rows]
    aF, Xc = np.repeat(alpha, D, axis=1), X[colidx].astype(np.float64)
    b = np.zeros(X.shape[1]) if bias is None else bias.astype(np.float64)
    Y = segsum(aF * Xc, rows, n) + b
    return dict(Y=np.maximum(Y, 0) if relu else Y, rowmax=m, rowsum=z, alpha=alpha, S_Y=segsum(aF * np.abs(Xc), rows, n) + np.abs(b))


def backward(rowptr, colidx, H, slope, G, X, Y, bias, rowterm, colterm, rowmax, rowsum, dot=None):
    """The closed form of both backward calls from the float32 operands THEY are handed, on one pattern (row i, column c):
    dot, drowterm (row side; dot = <G, Y - bias> per head) and, with `dot` given, dX, dcolterm (column side, taken over the pattern's
    columns) -- with S_* for each."""
    rows, n = row_of_entries(rowptr), len(rowptr) - 1
    nc, F = X.shape
    D = F // H
    heads = lambda a: a.reshape(a.shape[0], H, D).sum(2)  # noqa: E731
    t, _, _ = scores(rowptr, colidx, rowterm, colterm, slope)
    e = np.where(t > 0, t, t * np.float32(slope)).astype(np.float32)
    alpha = np.exp((e - rowmax[rows]).astype(np.float32).astype(np.float64)) / rowsum[rows].astype(np.float64)
    G64, X64 = G.astype(np.float64), X.astype(np.float64)
    out = {}
    if dot is None:
        b = np.zeros(F) if bias is None else bias.astype(np.float64)
        dot = heads(G64 * (Y.astype(np.float64) - b))
        S_dot = heads(np.abs(G64) * (np.abs(Y.astype(np.float64)) + np.abs(b)))
        out.update(dot=dot, S_dot=S_dot)
    else:
        dot, S_dot = dot.astype(np.float64), np.abs(dot.astype(np.float64))
    GX = G64[rows] * X64[colidx]
    dalpha, absda = heads(GX), heads(np.abs(GX))
    dt = alpha * (dalpha - dot[rows]) * np.where(t > 0, 1.0, float(np.float32(slope)))
    S_dt = alpha * (absda + S_dot[rows])
    aF = np.repeat(alpha, D, axis=1)
    out.update(drowterm=segsum(dt, rows, n), S_drowterm=segsum(S_dt, rows, n), dcolterm=segsum(dt, colidx, nc), S_dcolterm=segsum(S_dt, colidx, nc),
               dX=segsum(aF * G64[rows], colidx, nc), S_dX=segsum(aF * np.abs(G64[rows]), colidx, nc))
    return out


# ---- c of each bar, from the header's ORDER ------------------------------------------------------------------------------------------
def adds(d):
    """additions an entry's term goes through in a row sum of d entries: one accumulator over its segment, then the segments ascending"""
    d = np.asarray(d, dtype=np.int64)
    return np.minimum(d, SEG) + -(-d // SEG)


def dot_chain(D):
    """a head's dot product (gnnx_edge_dot.h, F := D): one product, 4 adds per chunk a lane owns, log2 G butterfly stages"""
    Q = -(-D // 4)
    G = 1
    while G < Q and G < 64:
        G <<= 1
    return 1 + 4 * -(-Q // G) + int(np.log2(G))


def c_rowsum(d):      # expf, the adds
    return 4 + adds(d)


def c_Y(d):           # N: expf, product, adds;  z: c_rowsum, carried by |Y0| <= S;  the division;  the bias
    return (4 + 1 + adds(d)) + c_rowsum(d) + 2


def c_dot(D):         # Y - bias, then the dot's chain
    return 1 + dot_chain(D)


def c_dterm(d, D):    # alpha: expf + division (m, z are operands);  dalpha - dot, * alpha, * slope;  the worse of dalpha and dot;  adds
    return 5 + 3 + c_dot(D) + adds(d)


def c_dX(d):          # alpha: expf + division;  the product;  adds;  beta
    return 5 + 1 + adds(d) + 1
