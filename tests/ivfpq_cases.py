"""Expected values of the ADC scan (mevi_ivfpq_scan_topk_f32) from existing oracle calls only, and the small generators the
IVF-PQ tests share.  No number here is a tolerance: the bar of the GPU tests is bit equality (scores as uint32, ids equal).

`adc_expected` restates include/mevi_hip_ivfpq.h:
  lut[j] = oracle.dense.pair_dot(q[j * dsub:(j + 1) * dsub], codebook[j])            the sequential fmaf chain from +0
  score  = ((bias + lut[0][code_0]) + lut[1][code_1]) + ...                           np.float32 array adds, ascending j
  probes : an entry outside [0, nlist) is empty, a list named twice counts once, at its FIRST slot and with that slot's bias
  a list is scanned up to max_list_len rows
  result : np.lexsort((ids, -scores))[:k], padded with -FLT_MAX / -1; ids compare as unsigned 32-bit values."""
import numpy as np

from oracle import dense as odense


def luts_by_pair_dot(q, codebook):
    """f32 [nq, m, K] lookup tables, entry by entry: lut[i, j] = oracle.dense.pair_dot(q_i's slice j, codebook[j]).  One foreign call
    per entry: for small cases."""
    q = np.ascontiguousarray(q, np.float32)
    cb = np.ascontiguousarray(codebook, np.float32)
    m, K, dsub = cb.shape
    assert q.shape[1] == m * dsub
    out = np.empty((len(q), m, K), np.float32)
    for i in range(len(q)):
        for j in range(m):
            out[i, j] = odense.pair_dot(q[i, j * dsub:(j + 1) * dsub], cb[j])
    return out


def luts(q, codebook):
    """The same tables with one oracle call per subspace: oracle.dense.ip_topk_exact of all query slices against codebook[j] with
    k = K returns every one of the K chains (the same pinned fmaf chain from +0 as pair_dot; tests/test_ivfpq_cpu.py holds the two
    routes equal bit for bit), sorted; they are put back by centroid."""
    q = np.ascontiguousarray(q, np.float32)
    cb = np.ascontiguousarray(codebook, np.float32)
    m, K, dsub = cb.shape
    assert q.shape[1] == m * dsub
    out = np.empty((len(q), m, K), np.float32)
    for j in range(m):
        s, c = odense.ip_topk_exact(q[:, j * dsub:(j + 1) * dsub], cb[j], K)
        assert (np.sort(c, axis=1) == np.arange(K)).all()
        np.put_along_axis(out[:, j, :], c, s, axis=1)
    return out


def adc_scores(lut, codes, bias):
    """Scores of the rows `codes` u8 [n, m] under one query's table f32 [m, K]: sequential f32 adds from `bias`."""
    acc = np.full(len(codes), bias, np.float32)
    for j in range(lut.shape[0]):
        acc = acc + lut[j][codes[:, j]]
        assert acc.dtype == np.float32
    return acc


def clean_slots(row, nlist):
    """[(slot, list)] of one probe row that survive: in range, first mention."""
    seen, out = set(), []
    for s, l in enumerate(np.asarray(row).tolist()):
        if 0 <= l < nlist and l not in seen:
            seen.add(l)
            out.append((s, l))
    return out


def adc_expected(q, codebook, codes, offsets, row_ids, probe, probe_score, k, max_list_len=None):
    """(scores f32 [nq, k], ids i64 [nq, k]).  codes u8 [nd, m] list-major, offsets i64 [nlist + 1], row_ids i64 [nd] or None (the
    id is the list-major row), probe [nq, nprobe], probe_score f32 [nq, nprobe] or None (+0)."""
    codes, offsets = np.asarray(codes), np.asarray(offsets, np.int64)
    nlist = len(offsets) - 1
    table = luts(q, codebook)
    out_s = np.full((len(q), k), -odense.FLT_MAX, np.float32)
    out_i = np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        scores, ids = [], []
        for s, l in clean_slots(probe[i], nlist):
            a, b = int(offsets[l]), int(offsets[l + 1])
            if max_list_len is not None:
                b = min(b, a + max_list_len)
            if b <= a:
                continue
            bias = np.float32(0.0) if probe_score is None else np.float32(probe_score[i, s])
            scores.append(adc_scores(table[i], codes[a:b], bias))
            rows = np.arange(a, b, dtype=np.int64)
            ids.append(rows if row_ids is None else np.asarray(row_ids, np.int64)[a:b])
        if not scores:
            continue
        scores, ids = np.concatenate(scores), np.concatenate(ids)
        best = np.lexsort((ids, -scores))[:k]
        out_s[i, :len(best)], out_i[i, :len(best)] = scores[best], ids[best]
    return out_s, out_i


def adc_float64(q, codebook, codes, bias):
    """Float64 ADC of one query over rows `codes`: bias + sum_j <q_j, codebook[j][code_j]>, for checking the reference."""
    cb = np.asarray(codebook, np.float64)
    m, _, dsub = cb.shape
    qs = np.asarray(q, np.float64).reshape(m, dsub)
    return np.float64(bias) + sum((cb[j][codes[:, j]] * qs[j]).sum(1) for j in range(m))


def random_index(seed, dim, m, K, nq, nd, nlist, nprobe, lens=None, repeats=False):
    """A random index given directly: (q, codebook, codes list-major, offsets, row_ids = a permutation, probe, probe_score).  The
    probe rows name distinct lists, or with `repeats` independent draws (a list may come twice in a row)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    codebook = rng.standard_normal((m, K, dim // m)).astype(np.float32)
    if lens is None:
        list_of = np.sort(rng.integers(0, nlist, size=nd))
        lens = np.bincount(list_of, minlength=nlist)
    lens = np.asarray(lens, np.int64)
    nd = int(lens.sum())
    offsets = np.zeros(nlist + 1, np.int64)
    offsets[1:] = np.cumsum(lens)
    codes = rng.integers(0, K, size=(nd, m)).astype(np.uint8)
    row_ids = np.concatenate([np.sort(c) for c in np.split(rng.permutation(nd).astype(np.int64), offsets[1:-1])]) if nd else np.zeros(0, np.int64)
    probe = (rng.integers(0, nlist, size=(nq, nprobe)) if repeats else np.stack([rng.permutation(nlist)[:nprobe] for _ in range(nq)])).astype(np.int32)
    probe_score = rng.standard_normal((nq, nprobe)).astype(np.float32)
    return q, codebook, codes, offsets, row_ids, probe, probe_score
