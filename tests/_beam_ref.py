"""Beam search's decoding rule (whisper.py's module docstring, "Beam search"), restated loop by loop in plain Python /
numpy for the tests: sorting with Python's ``sorted`` and the pool as a list, nothing shared with the kernels.

``BeamRef(B, K, L1, ...)`` holds the state of one generate call: prefixes, running sums, pools, done flags.  ``step`` takes
each row's candidates (ids and log-probabilities, [B*K, N], N >= 2K); ``finalize`` ends the call.  ``dtype`` np.float32
reproduces the kernels' arithmetic (an fp32 add per candidate, fp32 t ** length_penalty rounded once, correctly rounded
divisions) bit for bit; np.float64 is the exact-arithmetic reading.  ``run`` drives it from a function that returns
full log-probability rows."""
import numpy as np


def len_pow(n, length_penalty, dtype=np.float32):
    return dtype(float(n) ** float(length_penalty))


class BeamRef:
    def __init__(self, B, K, L1, start=50257, eos=2, length_penalty=1.0, early_stopping=False, dtype=np.float32):
        self.B, self.K, self.L1, self.eos, self.lp, self.early, self.dt = B, K, L1, eos, length_penalty, early_stopping, dtype
        self.prefix = [[start] for _ in range(B * K)]
        self.sums = [dtype(0.0) if r % K == 0 else dtype(-np.inf) for r in range(B * K)]
        self.pools = [[] for _ in range(B)]  # entries [score, insertion number, tokens]
        self.inserted = [0] * B
        self.done = [False] * B
        self.n_done = 0
        self.t = 0

    def _offer(self, b, score, tokens):
        pool = self.pools[b]
        if len(pool) == self.K:
            if not score > pool[-1][0]:
                return
            pool.pop()
        pool.append([score, self.inserted[b], list(tokens)])
        self.inserted[b] += 1
        pool.sort(key=lambda e: (-e[0], e[1]))

    def step(self, cand_ids, cand_lp):
        """One decoding step; cand_ids / cand_lp [B*K, N] (numpy)."""
        self.t += 1
        t, K, dt = self.t, self.K, self.dt
        den = len_pow(t, self.lp, dt)
        new_prefix = [list(p) for p in self.prefix]
        for b in range(self.B):
            if self.done[b]:
                continue
            cands = []
            for k in range(K):
                r = b * K + k
                for j in range(cand_ids.shape[1]):
                    v = int(cand_ids[r, j])
                    cands.append((dt(self.sums[r] + dt(cand_lp[r, j])), k, v))
            cands.sort(key=lambda c: (-c[0], c[1], c[2]))
            live = []
            for j, (score, k, v) in enumerate(cands[:2 * K]):
                if self.eos >= 0 and v == self.eos:
                    if j < K:
                        self._offer(b, dt(score / den), self.prefix[b * K + k] + [v])
                    continue
                if len(live) < K:
                    live.append((score, k, v))
            for n, (score, k, v) in enumerate(live):
                new_prefix[b * K + n] = self.prefix[b * K + k] + [v]
                self.sums[b * K + n] = score
            if len(self.pools[b]) == K and (self.early or self.pools[b][-1][0] >= dt(live[0][0] / den)):
                self.done[b] = True
                self.n_done += 1
        self.prefix = new_prefix

    def finalize(self):
        n = self.t
        den = len_pow(n, self.lp, self.dt)
        for b in range(self.B):
            if self.done[b]:
                continue
            for k in range(self.K):
                r = b * self.K + k
                self._offer(b, self.dt(self.sums[r] / den), self.prefix[r])

    def output(self, R, pad=0):
        """(sequences [B*R] lists, scores [B*R], lengths [B*R])."""
        seqs, scores, lens = [], [], []
        for b in range(self.B):
            for score, _, toks in self.pools[b][:R]:
                seqs.append(list(toks))
                scores.append(score)
                lens.append(len(toks) - 1)
        return seqs, scores, lens

    def padded(self, R, pad=0):
        seqs, _, lens = self.output(R)
        width = 1 + max(lens)
        return np.array([s + [pad] * (width - len(s)) for s in seqs], dtype=np.int64)


def top_candidates(lp_rows, N):
    """Each row's N best columns, ordered by log-probability desc then column asc: (ids [R, N], lps [R, N])."""
    ids = np.empty((len(lp_rows), N), dtype=np.int64)
    for r, row in enumerate(lp_rows):
        order = sorted(range(len(row)), key=lambda v: (-row[v], v))[:N]
        ids[r] = order
    lps = np.take_along_axis(np.asarray(lp_rows), ids, axis=1)
    return ids, lps


def run(lp_fn, B, K, max_length, R=1, start=50257, eos=2, length_penalty=1.0, early_stopping=False, dtype=np.float64,
        after_step=None):
    """The whole call: ``lp_fn(prefixes)`` -> log-probability rows [B*K, V] for the B*K current prefixes.  Returns the
    finished BeamRef (``.t`` is the number of steps run).  ``after_step(ref, cand_ids, cand_lps)`` sees every step."""
    ref = BeamRef(B, K, 1 + max_length, start, eos, length_penalty, early_stopping, dtype)
    for _ in range(max_length):
        lp = np.asarray(lp_fn([list(p) for p in ref.prefix]), dtype=np.float64)
        ids, lps = top_candidates(lp, 2 * K)
        ref.step(ids, lps)
        if after_step is not None:
            after_step(ref, ids, lps)
        if ref.n_done == B:
            break
    ref.finalize()
    return ref
