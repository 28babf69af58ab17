"""What the OPQ tests share (mevi_amd/opq.py, include/mevi_hip_opq.h): two anisotropic corpora, a float64 numpy restatement of the
rotation trainer with the flat ADC recall it is judged by, the expected value of mevi_opq_rotate_rows_f32 from the oracle's
pinned chain, and the refusal table of that entry point (it needs no GPU: every refusal comes before the launch).

`rotate_expected` restates include/mevi_hip_opq.h:
  out[i][o] = oracle.dense.pair_dot(x[rows[i]], R)[o] - crot[list_of[rows[i]]][o]     the chain, then one np.float32 subtraction
  a row id outside [0, n_src) or a list outside [0, nlist) gives a row of zeros."""
import numpy as np

from oracle import dense as odense

INVALID, UNSUPPORTED = -1, -2


# ---- corpora ------------------------------------------------------------------------------------------------------------
def outlier_rows(seed, n, dim):
    """Gaussian rows whose first four dimensions have standard deviation 6 and the others 1: the outlier dimensions of a dense
    retriever's embeddings, all of them inside the first subspace of a product quantiser."""
    scale = np.ones(dim)
    scale[:4] = 6.0
    return (np.random.default_rng(seed).standard_normal((n, dim)) * scale).astype(np.float32)


def decaying_rows(seed, n, dim):
    """Gaussian rows with standard deviation 0.85^d in dimension d: a spectrum that decays across the subspaces."""
    return (np.random.default_rng(seed).standard_normal((n, dim)) * 0.85 ** np.arange(dim)).astype(np.float32)


GENERATORS = {"outlier": outlier_rows, "decaying": decaying_rows}


# ---- the trainer in float64 -----------------------------------------------------------------------------------------------
def pq_assign64(Y, book):
    """codes i64 [n, M]: nearest centroid per subspace, lowest index on ties."""
    M, K, dsub = book.shape
    parts = Y.reshape(len(Y), M, dsub)
    return np.stack([((parts[:, j, None, :] - book[j][None]) ** 2).sum(-1).argmin(1) for j in range(M)], 1)


def pq_lloyd64(Y, book, iters):
    """`iters` Lloyd iterations of every subspace's k-means from `book`; an empty cluster keeps its old centre."""
    M, K, dsub = book.shape
    parts = Y.reshape(len(Y), M, dsub)
    book = book.copy()
    for _ in range(iters):
        codes = pq_assign64(Y, book)
        for j in range(M):
            counts = np.bincount(codes[:, j], minlength=K)
            sums = np.zeros((K, dsub))
            np.add.at(sums, codes[:, j], parts[:, j])
            live = counts > 0
            book[j][live] = sums[live] / counts[live, None]
    return book


def pq_decode64(codes, book):
    return np.concatenate([book[j][codes[:, j]] for j in range(book.shape[0])], 1)


def pq_error64(Y, book):
    """(||Y - Y^||^2 / n, codes)."""
    codes = pq_assign64(Y, book)
    return float(((Y - pq_decode64(codes, book)) ** 2).sum() / len(Y)), codes


def seed_book(Y, M, K, rng):
    """A codebook of K sampled rows' slices."""
    return Y[rng.permutation(len(Y))[:K]].reshape(K, M, -1).transpose(1, 0, 2).copy()


def random_rotation64(dim, rng):
    q, r = np.linalg.qr(rng.standard_normal((dim, dim)))
    return q * np.where(np.diag(r) < 0, -1.0, 1.0)[None, :]


def train_rotation64(X, M, K, niter, niter_pq_0=40, niter_pq=4, seed=0):
    """(R, errors, R_last, book): OPQMatrix::train in float64 -- rotate, k-means per subspace (hot-started after the first
    iteration), encode, Procrustes R = U V^T of svd(Y^^T X).  errors[t] belongs to the rotation and the codebook of iteration t:
    R_last and book are those of the last iteration, R the result of the Procrustes step after it (what the trainer returns)."""
    X = np.asarray(X, np.float64)
    rng = np.random.default_rng(seed)
    R = random_rotation64(X.shape[1], rng)
    errors, book = [], None
    for t in range(niter):
        R_last = R
        Y = X @ R.T
        if book is None:
            book = seed_book(Y, M, K, rng)
        book = pq_lloyd64(Y, book, niter_pq_0 if t == 0 else niter_pq)
        err, codes = pq_error64(Y, book)
        errors.append(err)
        U, _, Vt = np.linalg.svd(pq_decode64(codes, book).T @ X)
        R = U @ Vt
    return R, errors, R_last, book


def train_pq64(X, M, K, iters, seed=0):
    """Plain PQ on the unrotated rows: the same k-means, `iters` iterations from sampled rows."""
    X = np.asarray(X, np.float64)
    return pq_lloyd64(X, seed_book(X, M, K, np.random.default_rng(seed)), iters)


def recall_at(found, exact):
    """Mean fraction of every row of `exact` that `found` holds."""
    return float(np.mean([len(set(f.tolist()) & set(e.tolist())) / len(e) for f, e in zip(found, exact)]))


def adc_recall64(X, Q, R, book, k=10):
    """recall@k of flat ADC -- <R q, decode(encode(R x))> -- against the exact inner-product search (R None: no rotation)."""
    X, Q = np.asarray(X, np.float64), np.asarray(Q, np.float64)
    Y, Qr = (X, Q) if R is None else (X @ R.T, Q @ R.T)
    approx = Qr @ pq_decode64(pq_assign64(Y, book), book).T
    return recall_at(np.argsort(-approx, 1, kind="stable")[:, :k], np.argsort(-(Q @ X.T), 1, kind="stable")[:, :k])


# ---- the rotation kernel's expected value ---------------------------------------------------------------------------------
def rotate_expected(x, R, rows=None, list_of=None, crot=None):
    """f32 [n, dim] of the module docstring.  One oracle call per output element: for small cases."""
    x, R = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(R, np.float32)
    n_src, dim = x.shape
    assert R.shape == (dim, dim) and (list_of is None) == (crot is None)
    src = np.arange(n_src) if rows is None else np.asarray(rows, np.int64)
    out = np.zeros((len(src), dim), np.float32)
    chains = {}
    for i, r in enumerate(src.tolist()):
        if not 0 <= r < n_src:
            continue
        if crot is not None and not 0 <= int(list_of[r]) < len(crot):
            continue
        if r not in chains:
            chains[r] = odense.pair_dot(x[r], R)
        y = chains[r]
        if crot is not None:
            y = y - np.asarray(crot, np.float32)[int(list_of[r])]
        assert y.dtype == np.float32
        out[i] = y
    return out


def chain_bound(x, R, crot_row=None):
    """Bound of |chain(x, R) - crot - exact| per output: dim fmas (and one subtraction), each rounding at most 2^-24 of a partial
    sum bounded by the sum of absolute terms."""
    mag = np.abs(np.asarray(x, np.float64)) @ np.abs(np.asarray(R, np.float64)).T
    if crot_row is not None:
        mag = mag + np.abs(np.asarray(crot_row, np.float64))
    return (x.shape[-1] + 1) * 2.0 ** -24 * mag


# ---- refusals of mevi_opq_rotate_rows_f32, before any launch (fake pointers: nothing may dereference them) --------------------
def check_refusals(L):
    A = 1 << 20

    def call(x=A, n_src=100, dim=64, rows=A, n=50, list_of=A, crot=A, nlist=4, R=A, out=A):
        st = L.mevi_opq_rotate_rows_f32(x, n_src, dim, rows, n, list_of, crot, nlist, R, out, None)
        return st, L.mevi_last_error().decode()

    def refused(code, word, **kw):
        st, msg = call(**kw)
        assert st == code and word in msg and msg.startswith("opq_rotate:"), (kw, st, msg)

    refused(UNSUPPORTED, "dim=66", dim=66)
    refused(UNSUPPORTED, "dim=4100", dim=4100)
    refused(UNSUPPORTED, "n=", n=1 << 31)
    refused(INVALID, "n=-1", n=-1)
    refused(INVALID, "n_src=-1", n_src=-1)
    refused(INVALID, "dim=0", dim=0)
    refused(INVALID, "nlist=-1", nlist=-1)
    refused(INVALID, "n=101", n=101, rows=None)
    refused(INVALID, "crot", crot=None)
    refused(INVALID, "crot", list_of=None)
    refused(INVALID, "nlist=0", nlist=0)
    for name in ("x", "R", "out"):
        refused(INVALID, "null", **{name: None})
    for name, step in (("x", 8), ("crot", 4), ("R", 8), ("out", 4), ("rows", 4), ("list_of", 2)):
        refused(INVALID, "align", **{name: A + step})
    assert call(n=0, x=None, out=None, rows=None)[0] == 0                 # nothing to do: no launch, nothing dereferenced
    assert call(n=0, list_of=None, crot=None, nlist=0)[0] == 0
    assert call(n=0, dim=66)[0] == UNSUPPORTED                           # ... but the envelope still holds
