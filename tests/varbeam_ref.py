"""Plain Python/NumPy restatement of the variable-depth beam search (mevi_beam_step_var_f32 / mevi_beam_finalize_var_f32),
written from the reference's own loop -- MEVI/transformers/generation_utils.py:783-1001 (step, flush, output) and
BeamHypotheses :1268-1315 -- over a dict trie as TreeBuilder builds it (MEVI/main_models.py:50-69).

Float order: candidate = f32(beam score) + f32(log-softmax) (one f32 add, `dtype` = np.float64 for the error study);
hypothesis score = float(candidate) / cur_len ** length_penalty in Python floats, as the reference computes it.
Candidates are ordered (score descending, flat index beam * (K + 1) + column ascending; column 0 = eos)."""
import numpy as np


class Trie:
    __slots__ = ("children", "end", "index")

    def __init__(self):
        self.children, self.end, self.index = {}, False, None      # index: position in its level (set by trie_levels)


def build_trie(paths, cutoff=None):
    """Brute-force trie of code sequences; `end` = an id ends at the node (TreeBuilder.add's eos child)."""
    root = Trie()
    for path in paths:
        cur = root
        for c in list(path)[:cutoff]:
            cur = cur.children.setdefault(int(c), Trie())
        cur.end = True
    return root


def trie_levels(root, K, n_levels):
    """The level arrays RaggedPrefixTree must produce: per level (mask u32 [n, W], base i32 [n], ends u8 [n]) with the
    nodes of a level in lexicographic order of their prefixes; plus the node count of every level 0 .. n_levels."""
    W = (K + 31) // 32
    level, out, counts = [root], [], []
    for _ in range(n_levels):
        counts.append(len(level))
        mask = np.zeros((max(len(level), 1), W), np.uint32)
        base = np.zeros(max(len(level), 1), np.int32)
        ends = np.zeros(max(len(level), 1), np.uint8)
        nxt = []
        for i, nd in enumerate(level):
            nd.index = i
            ends[i] = nd.end
            if nd.children:
                base[i] = len(nxt)
            for c in sorted(nd.children):
                mask[i, c >> 5] |= np.uint32(1 << (c & 31))
                nxt.append(nd.children[c])
        out.append((mask, base, ends))
        level = nxt
    counts.append(len(level))
    for i, nd in enumerate(level):
        nd.index = i
    return out, counts


def log_softmax_wave(row):
    """(x - max) - log(sum exp(x - max)) in f32 with the kernel's summation order: lane l adds columns l, l + 64, ...,
    then the 64 lanes fold by xor 32, 16, ..., 1."""
    x = np.asarray(row, np.float32)
    m = x.max()
    e = np.exp(x - m, dtype=np.float32)
    lanes = np.zeros(64, np.float32)
    for c in range(x.size):
        lanes[c & 63] = np.float32(lanes[c & 63] + e[c])
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[idx ^ off]).astype(np.float32)
    return ((x - m) - np.log(lanes[0], dtype=np.float32)).astype(np.float32)


class Hypotheses:
    """BeamHypotheses (early_stopping=False) with the list order kept: entries are [score, insertion number, tokens]."""

    def __init__(self, R, length_penalty):
        self.R, self.lp, self.beams, self.worst, self.inserted = R, length_penalty, [], 1e9, 0

    def add(self, tokens, sum_logp):
        score = float(sum_logp) / len(tokens) ** self.lp
        if len(self.beams) < self.R or score > self.worst:
            self.beams.append([score, self.inserted, list(tokens)])
            self.inserted += 1
            if len(self.beams) > self.R:
                order = sorted((b[0], i) for i, b in enumerate(self.beams))
                del self.beams[order[0][1]]
                self.worst = order[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logp, cur_len):
        if len(self.beams) < self.R:
            return False
        return self.worst >= float(best_sum_logp) / cur_len ** self.lp


class Query:
    """One query's search state: R open beams (scores, trie nodes -- None = off the tree --, token prefixes), its pool."""

    def __init__(self, root, R, K, T, length_penalty, dtype=np.float32):
        self.R, self.K, self.T, self.dtype = R, K, T, dtype
        self.scores = np.zeros(R, dtype)
        self.scores[1:] = -1e9
        self.nodes = [root] * R
        self.prefix = [[0] for _ in range(R)]
        self.pool = Hypotheses(R, length_penalty)
        self.done = False
        self.parent = self.code = None

    def candidates(self, lsm):
        cand = np.full((self.R, self.K + 1), -np.inf, self.dtype)
        lsm = np.asarray(lsm).astype(self.dtype)
        for r, nd in enumerate(self.nodes):
            if nd is None:
                continue
            if nd.end:
                cand[r, 0] = self.scores[r] + lsm[r, 0]
            for c in nd.children:
                cand[r, 1 + c] = self.scores[r] + lsm[r, 1 + c]
        return cand

    def step(self, p, lsm):
        """lsm [R, K+1]: the log-softmax rows of the R beams at position p (column 0 = eos)."""
        R, K = self.R, self.K
        flat = self.candidates(lsm).reshape(-1)
        top = sorted(range(flat.size), key=lambda i: (-flat[i], i))[:2 * R]
        nxt = []
        for rank, i in enumerate(top):
            r, col = divmod(i, K + 1)
            if col == 0:
                if rank >= R:
                    continue
                if not self.done:
                    self.pool.add(self.prefix[r], flat[i])
            else:
                nxt.append((flat[i], r, col - 1))
            if len(nxt) == R:
                break
        if not self.done:
            self.done = self.pool.is_done(flat[top[0]], p + 1)
        assert len(nxt) == R
        self.scores = np.array([s for s, _, _ in nxt], self.dtype)
        self.parent = [r for _, r, _ in nxt]
        self.code = [c for _, _, c in nxt]
        nodes, prefix = [], []
        for s, r, c in nxt:
            nd = self.nodes[r]
            nodes.append(nd.children.get(c) if nd is not None else None)
            prefix.append(self.prefix[r] + [2 + p * K + c])
        self.nodes, self.prefix = nodes, prefix

    def finalize(self):
        """-> (decoded [R, T], scores [R], lengths [R]): the flush of a query that is not done, then the pool best first."""
        if not self.done:
            for r in range(self.R):
                self.pool.add(self.prefix[r], self.scores[r])
        hyps = sorted(self.pool.beams, key=lambda b: b[0])
        decoded = np.zeros((self.R, self.T), np.int64)
        scores, lengths = [], []
        for j in range(self.R):
            score, _, tokens = hyps.pop()
            decoded[j, :len(tokens)] = tokens
            if len(tokens) < self.T:
                decoded[j, len(tokens)] = 1
            scores.append(score)
            lengths.append(len(tokens))
        return decoded, np.array(scores, np.float64), np.array(lengths, np.int32)


def search(root, step_lsm, B, R, K, T, length_penalty, dtype=np.float32):
    """Run B queries for T - 1 steps.  step_lsm(p, queries) -> [B, R, K+1] log-softmax rows of position p (it may read the
    queries' prefixes / parents to produce them).  -> (decoded [B*R, T], scores [B*R], lengths [B*R], queries)."""
    qs = [Query(root, R, K, T, length_penalty, dtype) for _ in range(B)]
    for p in range(T - 1):
        lsm = step_lsm(p, qs)
        for b, q in enumerate(qs):
            q.step(p, lsm[b])
    outs = [q.finalize() for q in qs]
    return (np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]),
            np.concatenate([o[2] for o in outs]), qs)


def oracle_search(W, cfg, ids, mask, R, paths, length_penalty=0.8, dtype=np.float32):
    """The restatement driven by the torch-fp32 oracle model (oracle.t5, as the base-shape test of the fixed-depth search
    drives its restatement): every step's logits come from oracle.t5.nci_last_logits on the restatement's OWN prefixes,
    log-softmax over the whole decode vocabulary as the reference takes it.  -> (decoded [B*R, T], scores, lengths)."""
    import torch
    import torch.nn.functional as F

    from oracle import t5 as ot5

    M, K = cfg["M"], cfg["K"]
    root = build_trie(paths)
    enc = ot5.encoder(W, cfg, ids, mask)
    outs = []
    for b in range(ids.shape[0]):
        e, m = enc[b:b + 1].expand(R, -1, -1), mask[b:b + 1].expand(R, -1)
        q = Query(root, R, K, M + 2, length_penalty, dtype)
        for p in range(M + 1):
            logits = ot5.nci_last_logits(W, cfg, torch.tensor(q.prefix, dtype=torch.long), e, m)
            cols = [1] + list(range(2 + p * K, 2 + (p + 1) * K))
            q.step(p, F.log_softmax(logits, dim=-1)[:, cols].numpy())
        outs.append(q.finalize())
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), np.concatenate([o[2] for o in outs])


def near_tie_swaps(got, want, want_scores, R, tol):
    """Rows of `got` that differ from `want` at their rank must be `want`'s row of a rank whose score is within `tol` of
    that rank's (a swap inside a near-tie); anything else raises.  -> number of such rows."""
    B = got.shape[0] // R
    got, want, sc = got.reshape(B, R, -1), want.reshape(B, R, -1), want_scores.reshape(B, R)
    swapped = 0
    for i in range(B):
        for j in range(R):
            if (got[i, j] == want[i, j]).all():
                continue
            twins = [jj for jj in range(R) if (got[i, j] == want[i, jj]).all()]
            assert twins and abs(sc[i, twins[0]] - sc[i, j]) < tol, (i, j, twins, sc[i].tolist())
            swapped += 1
    return swapped
