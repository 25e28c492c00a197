"""A NumPy restatement of the neighbour sampler (gnnx_csr_sample_neighbors, include/gnnx.h "neighbour sampling"), independent of the
kernels: entry j of row i has the key u_j = (h_j >> 32) << 32 | j with h_j = splitmix64(splitmix64(seed) ^ ((i << 32 | j) * golden)); a
row of d <= k entries keeps them all, a longer one the k entries with the smallest u_j, in stored order.  The keys of a row are
pairwise different, so a sort of the uint64 keys needs no tie rule.  `sample_row_segmented` restates the hub path's claim: the k
smallest of a row are the k smallest of the per-segment k smallest.  tests/test_sample_cpu.py pins the finaliser to synth.splitmix64
and checks the draw's uniformity."""
import numpy as np

SEG = 4096   # S of the contract
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def finaliser(x):
    """splitmix64 of a uint64 array, written out on its own (tests/test_sample_cpu.py holds it against synth.splitmix64)."""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def keys(seed, i, d):
    """u_0 .. u_{d-1} of row i as uint64."""
    j = np.arange(d, dtype=np.uint64)
    s = finaliser(np.uint64(int(seed) & MASK64))
    with np.errstate(over="ignore"):
        h = finaliser(s ^ (((np.uint64(i) << np.uint64(32)) | j) * np.uint64(GOLDEN)))
    return ((h >> np.uint64(32)) << np.uint64(32)) | j


def smallest(u, k):
    """Ascending positions of the min(k, len(u)) smallest of the pairwise different keys u."""
    if len(u) <= k:
        return np.arange(len(u), dtype=np.int64)
    return np.sort(np.argsort(u, kind="stable")[:k])


def sample_row(seed, i, d, k):
    """Ascending offsets j of the kept entries of row i."""
    return smallest(keys(seed, i, d), k)


def sample_row_segmented(seed, i, d, k, S=SEG):
    """The same set by segments of S consecutive entries: each segment's min(k, len) smallest, then the k smallest of the candidates."""
    u = keys(seed, i, d)
    cand = np.concatenate([b + smallest(u[b:b + S], k) for b in range(0, d, S)]) if d else np.zeros(0, dtype=np.int64)
    return cand[smallest(u[cand], k)]


def sample_ref(rowptr, colidx, k, seed):
    """(rowptr', colidx', pos, rowid) as int32: the sampled CSR, the absolute input position and the row of every kept entry."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    colidx = np.asarray(colidx)
    n = len(rowptr) - 1
    pos, rowid = [], []
    for i in range(n):
        b, d = rowptr[i], rowptr[i + 1] - rowptr[i]
        j = sample_row(seed, i, int(d), k)
        pos.append(b + j)
        rowid.append(np.full(len(j), i, dtype=np.int64))
    pos = np.concatenate(pos).astype(np.int64) if n else np.zeros(0, dtype=np.int64)
    rowid = np.concatenate(rowid) if n else np.zeros(0, dtype=np.int64)
    rowptr_o = np.concatenate([[0], np.cumsum(np.minimum(np.diff(rowptr), k))]).astype(np.int32)
    return rowptr_o, colidx[pos].astype(np.int32), pos.astype(np.int32), rowid.astype(np.int32)
