"""Beam search on the GPU: tmi_lm_head_topk against an fp64 restatement, tmi_beam_step against tests/_beam_ref.py bit for
bit, ``generate(num_beams=...)`` on the reduced model against the reference rule driven by the oracle's fp64 logits and
against teacher-forced scores, greedy unchanged at num_beams=1, non-interference with training, ``transcribe_audio``
with beams and the full-size decode."""
import math

import numpy as np
import pytest
import torch

import _beam_ref as BR
from _margins import within

pytestmark = pytest.mark.gpu

V, VP = 51865, 51904
_RED = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, encoder_layers=2,
            decoder_layers=2)


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, whisper
    from oracle import whisper_oracle as O
    return ops, whisper, O


# ----------------------------------------------------------------------------- 1. tmi_lm_head_topk
def _ref_scaled(x, gamma, beta, eps, w, temperature):
    """fp64: s = (LayerNorm(x) . w)[:, :V] / T, its logsumexp, and the rounding scale sum_k |y_k w_kn| / T per row."""
    y = x.double()
    if gamma is not None:
        mu = y.mean(1, keepdim=True)
        var = ((y - mu) ** 2).mean(1, keepdim=True)
        y = (y - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    wd = w[:, :V].double()
    s = (y @ wd) / temperature
    return s, torch.logsumexp(s, 1), (y.abs() @ wd.abs()).max(1).values / temperature


def _topk(ops, x, x_ld, w, M, d, N, gamma=None, beta=None, temperature=1.0, ws=None, Vr=V):
    dev = w.device
    ids = torch.full((M, N), -7, dtype=torch.int32, device=dev)
    lp = torch.full((M, N), float("nan"), device=dev)
    lse = torch.empty(M, device=dev)
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, Vr, N), dtype=torch.int64, device=dev) if ws is None else ws
    ops.lm_head_topk(x, x_ld, w, VP, M, d, Vr, N, ids, lp, ws, gamma=gamma, beta=beta, temperature=temperature, lse=lse)
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0, "the workspace is not left zero"
    return ids, lp, lse


def _check_topk(ids, lp, lse, s, lse64, scale, rel, name):
    N = ids.shape[1]
    ids, lp = ids.long().cpu(), lp.double().cpu()
    s, lse64, scale = s.cpu(), lse64.cpu(), scale.cpu()
    assert bool(((ids >= 0) & (ids < V)).all()), ids
    for r in range(ids.shape[0]):
        assert len(set(ids[r].tolist())) == N
    lp64 = s.gather(1, ids) - lse64[:, None]
    bound = rel * (scale + lse64.abs())
    unit = bound / rel
    within(f"lm_head_topk {name} |lp - lp64| / (scale + |lse|)", float(((lp - lp64).abs() / unit[:, None]).max()), rel)
    within(f"lm_head_topk {name} |lse - lse64| / (scale + |lse|)", float(((lse.double().cpu() - lse64).abs() / unit).max()), rel)
    assert bool((lp[:, 1:] <= lp[:, :-1]).all()), "not sorted"
    top = s.topk(N + 1, dim=1)
    vals = top.values
    for r in range(ids.shape[0]):
        for j in range(N):
            gap_prev = vals[r, j - 1] - vals[r, j] if j > 0 else math.inf
            gap_next = vals[r, j] - vals[r, j + 1]
            if min(gap_prev, gap_next) > 2 * bound[r]:
                assert int(ids[r, j]) == int(top.indices[r, j]), (name, r, j, ids[r], top.indices[r])


@pytest.mark.parametrize("wdt", ["bf16", "fp32"])
def test_lm_head_topk_matches_fp64(dev, wdt):
    ops, _, _ = _mods()
    g = torch.Generator(device=dev).manual_seed(11)
    T = 0.7
    for d in (128, 768, 1280):
        w = torch.zeros(d, VP, device=dev)
        w[:, :V] = torch.randn(d, V, device=dev, generator=g) * d ** -0.5
        w = w.to(torch.bfloat16) if wdt == "bf16" else w
        xdt = torch.bfloat16 if wdt == "bf16" else torch.float32
        gamma = 1 + 0.1 * torch.randn(d, device=dev, generator=g)
        beta = 0.1 * torch.randn(d, device=dev, generator=g)
        for M in (1, 5, 16, 17, 40):
            full = (torch.randn(M * 3, d, device=dev, generator=g) * 2 + 0.5).to(xdt)
            x = full[2:]  # the last of every 3 positions, read in place
            s, lse64, scale = _ref_scaled(full[2::3], gamma, beta, 1e-5, w, T)
            for N in (1, 2, 10, 16):
                ids, lp, lse = _topk(ops, x, 3 * d, w, M, d, N, gamma, beta, temperature=T)
                _check_topk(ids, lp, lse, s, lse64, scale, 3e-7, f"{wdt} d{d} M{M} N{N} LN")
            s2, lse2, scale2 = _ref_scaled(full[2::3], None, None, 0.0, w, 1.0)
            ids, lp, lse = _topk(ops, x, 3 * d, w, M, d, 10)
            _check_topk(ids, lp, lse, s2, lse2, scale2, 3e-7, f"{wdt} d{d} M{M} plain")


def test_lm_head_topk_ties_pads_repeats_and_long_lists(dev):
    ops, _, _ = _mods()
    g = torch.Generator(device=dev).manual_seed(12)
    d, M, N = 768, 8, 10
    w32 = torch.zeros(d, VP, device=dev)
    w32[:, :V] = torch.randn(d, V, device=dev, generator=g) * d ** -0.5
    x = torch.randn(M, d, device=dev, generator=g)
    for wdt in (torch.float32, torch.bfloat16):
        w = w32.to(wdt)
        ids0, _, _ = _topk(ops, x.to(wdt), d, w, M, d, N)
        a = int(ids0[0, 0])
        # a copy of row 0's winner in a smaller column (another workgroup) ties: the smaller column comes first
        b = 3 if a > 3 else V - 1
        w2 = w.clone()
        w2[:, b] = w2[:, a]
        ids, lp, _ = _topk(ops, x.to(wdt), d, w2, M, d, N)
        assert ids[0, :2].tolist() == [min(a, b), max(a, b)] and float(lp[0, 0]) == float(lp[0, 1])
        # a row of equal logits (x = 0): columns 0 .. N-1, every log-probability -log V
        xz = x.clone()
        xz[3] = 0
        ids, lp, lse = _topk(ops, xz.to(wdt), d, w, M, d, N)
        assert ids[3].tolist() == list(range(N))
        assert abs(float(lp[3, 0]) + math.log(V)) < 1e-5
        # bit-identical repeats
        again = _topk(ops, x.to(wdt), d, w, M, d, N)
        first = _topk(ops, x.to(wdt), d, w, M, d, N)
        assert all(torch.equal(p, q) for p, q in zip(again, first))
    # all real logits negative: the zero pad columns [V, VP) are never chosen
    wneg = torch.zeros(d, VP, device=dev)
    wneg[:, :V] = -(torch.rand(d, V, device=dev, generator=g) + 0.1)
    xp = torch.rand(M, d, device=dev, generator=g) + 0.1
    ids, lp, lse = _topk(ops, xp, d, wneg, M, d, 16)
    assert bool((ids < V).all())
    s, lse64, scale = _ref_scaled(xp, None, None, 0.0, wneg, 1.0)
    _check_topk(ids, lp, lse, s, lse64, scale, 3e-7, "all-negative")
    # every workgroup holds 15 large logits and a small 16th: the largest lists that can meet at the end (15 x 16 keys)
    wl = torch.zeros(128, VP, device=dev)
    col = torch.arange(V, device=dev)
    wl[0, :V] = torch.where(col % 128 < 15, 10.0 + col * 1e-4, -10.0 - col * 1e-4)
    xl = torch.zeros(2, 128, device=dev)
    xl[:, 0] = 1.0
    ids, lp, lse = _topk(ops, xl, 128, wl, 2, 128, 16)
    s, lse64, scale = _ref_scaled(xl, None, None, 0.0, wl, 1.0)
    assert ids[0].tolist() == s[0].topk(16).indices.tolist()
    _check_topk(ids, lp, lse, s, lse64, scale, 3e-7, "long lists")
    # back to back on one workspace, no synchronisation between the calls
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, N), dtype=torch.int64, device=dev)
    wb = w32.to(torch.bfloat16)
    xs = [torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16) for _ in range(3)]
    outs = [(torch.empty(M, N, dtype=torch.int32, device=dev), torch.empty(M, N, device=dev)) for _ in range(3)]
    for xi, (oi, ol) in zip(xs, outs):
        ops.lm_head_topk(xi, d, wb, VP, M, d, V, N, oi, ol, ws)
    torch.cuda.synchronize()
    assert int(ws.abs().sum()) == 0
    for xi, (oi, ol) in zip(xs, outs):
        ids, lp, _ = _topk(ops, xi, d, wb, M, d, N)
        assert torch.equal(ids, oi) and torch.equal(lp, ol)


def test_lm_head_topk_rejects_bad_arguments(dev):
    ops, _, _ = _mods()
    from tethys_speech_amd._lib import TmiError
    d, M = 128, 2
    x = torch.randn(M, d, device=dev)
    w = torch.zeros(d, VP, device=dev)
    ids = torch.empty(M, 17, dtype=torch.int32, device=dev)
    lp = torch.empty(M, 17, device=dev)
    ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, 17), dtype=torch.int64, device=dev)
    short = ws[:ops.lm_head_topk_workspace_elems(M, V, 4) - 1]
    for kw in (dict(N=0), dict(N=17), dict(w_ld=V), dict(temperature=-1.0), dict(ws=short), dict(Vr=3)):
        a = dict(N=4, w_ld=VP, temperature=1.0, ws=ws, Vr=V)
        a.update(kw)
        with pytest.raises(TmiError):
            ops.lm_head_topk(x, d, w, a["w_ld"], M, d, a["Vr"], a["N"], ids, lp, a["ws"], temperature=a["temperature"])
    with pytest.raises(TmiError):
        ops.lm_head_topk(x, d, w, VP, M, d, V, 4, ids, lp, ws, gamma=torch.ones(d, device=dev))
    assert int(ws.abs().sum()) == 0


# ----------------------------------------------------------------------------- 2. tmi_beam_step
class DevBeam:
    def __init__(self, ops, dev, B, K, L1, start, eos, length_penalty, early):
        self.ops, self.B, self.K, self.L1, self.eos, self.lp, self.early = ops, B, K, L1, eos, length_penalty, early
        i32 = dict(dtype=torch.int32, device=dev)
        self.prefix = torch.full((2, B * K, L1), start, **i32)
        s = torch.zeros(B, K, device=dev)
        s[:, 1:] = float("-inf")
        self.sums = s.view(B * K)
        self.pool_ids = torch.full((B, K, L1), -5, **i32)
        self.pool_scores, self.pool_len = torch.zeros(B, K, device=dev), torch.zeros(B, K, **i32)
        self.pool_cnt, self.done, self.n_done = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(1, **i32)
        self.t = 0

    def step(self, ids, lps):
        self.t += 1
        t = self.t
        dev = self.sums.device
        ci = torch.as_tensor(ids, dtype=torch.int32).to(dev).contiguous()
        cl = torch.as_tensor(lps, dtype=torch.float32).to(dev).contiguous()
        self.ops.beam_step(ci, cl, ci.shape[1], self.B, self.K, self.sums, self.prefix[t & 1], self.prefix[(t + 1) & 1],
                           self.L1, t, self.eos, float(BR.len_pow(t, self.lp)), self.early, self.pool_ids, self.pool_scores,
                           self.pool_len, self.pool_cnt, self.done, self.n_done)

    def finalize(self):
        t = self.t
        self.ops.beam_step(None, None, 2 * self.K, self.B, self.K, self.sums, self.prefix[(t + 1) & 1], None, self.L1, t,
                           self.eos, float(BR.len_pow(t, self.lp)), self.early, self.pool_ids, self.pool_scores,
                           self.pool_len, self.pool_cnt, self.done, self.n_done, finalize=True)


def _same_state(db, ref, where):
    torch.cuda.synchronize()
    B, K, t = db.B, db.K, ref.t
    cur = db.prefix[(t + 1) & 1].cpu()
    sums = db.sums.cpu().numpy()
    for b in range(B):
        assert bool(db.done[b]) == ref.done[b], (where, b)
        for k in range(K):
            r = b * K + k
            n = len(ref.prefix[r])
            assert cur[r, :n].tolist() == ref.prefix[r], (where, r, cur[r, :n].tolist(), ref.prefix[r])
            assert sums[r].tobytes() == np.float32(ref.sums[r]).tobytes(), (where, r, sums[r], ref.sums[r])
        pool = ref.pools[b]
        assert int(db.pool_cnt[b]) == len(pool), (where, b)
        for p, (score, _, toks) in enumerate(pool):
            assert db.pool_scores[b, p].cpu().numpy().tobytes() == np.float32(score).tobytes(), (where, b, p)
            assert int(db.pool_len[b, p]) == len(toks) - 1, (where, b, p)
            assert db.pool_ids[b, p, :len(toks)].cpu().tolist() == toks, (where, b, p)
    assert int(db.n_done) == ref.n_done, where


def _synthetic_cands(rng, BK, N, Vs, eos, p_eos, quant):
    """Distinct ids per row, log-probabilities quantised to 1/quant (ties within and across rows)."""
    ids = np.stack([rng.choice(Vs, N, replace=False) for _ in range(BK)])
    if eos >= 0:
        hit = rng.random(BK) < p_eos
        for r in np.nonzero(hit)[0]:
            if eos not in ids[r]:
                ids[r, rng.integers(N)] = eos
    lps = -np.round(rng.exponential(1.0, (BK, N)) * quant) / quant
    return ids, lps.astype(np.float32)


@pytest.mark.parametrize("early,length_penalty", [(False, 1.0), (True, 1.0), (False, 0.0), (False, 2.0), (True, 0.5)])
def test_beam_step_matches_reference_bit_for_bit(dev, early, length_penalty):
    ops, _, _ = _mods()
    rng = np.random.default_rng(int(length_penalty * 10) + early)
    for B, K, N, eos, p_eos in ((3, 3, 6, 2, 0.5), (2, 8, 16, 5, 0.6), (4, 2, 4, 0, 0.9), (2, 4, 9, -1, 0.5)):
        L1 = 14
        db = DevBeam(ops, dev, B, K, L1, 77, eos, length_penalty, early)
        ref = BR.BeamRef(B, K, L1, 77, eos, length_penalty, early, np.float32)
        for t in range(1, L1 - 1):
            ids, lps = _synthetic_cands(rng, B * K, N, 40, eos, p_eos, 4 if t % 2 else 1000)
            db.step(ids, lps)
            ref.step(ids, lps)
            _same_state(db, ref, (B, K, t))
            if ref.n_done == B:
                # a step queued after the stop changes nothing
                ids, lps = _synthetic_cands(rng, B * K, N, 40, eos, p_eos, 4)
                db.step(ids, lps)
                ref.step(ids, lps)
                _same_state(db, ref, (B, K, t, "after stop"))
                break
        db.finalize()
        ref.finalize()
        _same_state(db, ref, (B, K, "finalize"))
        if eos < 0:
            assert ref.n_done == 0 and all(len(p) == K for p in ref.pools)


def test_beam_step_rejects_bad_arguments(dev):
    ops, _, _ = _mods()
    from tethys_speech_amd._lib import TmiError
    db = DevBeam(ops, dev, 2, 3, 8, 1, 2, 1.0, False)
    ids = torch.zeros(6, 6, dtype=torch.int32, device=dev)
    lp = torch.zeros(6, 6, device=dev)
    for kw in (dict(N=5), dict(K=9), dict(t=8), dict(t=0), dict(len_pow=0.0), dict(len_pow=float("inf"))):
        a = dict(N=6, K=3, t=1, len_pow=1.0)
        a.update(kw)
        with pytest.raises(TmiError):
            ops.beam_step(ids, lp, a["N"], 2, a["K"], db.sums, db.prefix[0], db.prefix[1], 8, a["t"], 2, a["len_pow"], False,
                          db.pool_ids, db.pool_scores, db.pool_len, db.pool_cnt, db.done, db.n_done)


# ----------------------------------------------------------------------------- model fixtures
_CACHE = {}


def _setup(T_in=3000, B=2):
    key = (T_in, B)
    if key not in _CACHE:
        _, whisper, O = _mods()
        ocfg = O.make_config("small", dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, **_RED)
        params = O.init_params(ocfg, seed=3, dtype=torch.float64)
        feats = torch.from_numpy(np.random.default_rng(T_in).standard_normal((B, 80, T_in)).astype(np.float32))
        enc = O.encoder(params, feats.double(), ocfg, training=False)
        _CACHE[key] = (ocfg, params, feats, enc)
    return _CACHE[key]


def _model(dev, precision, params, seed=1234):
    _, whisper, _ = _mods()
    m = whisper.create_whisper_model("small", device=dev, precision=precision, seed=seed, **_RED)
    m.arena.load_ref({k: v.float() for k, v in params.items()})
    m.refresh_shadows()
    return m


def _teacher_scores(model, feats, seqs, lens, R, T, length_penalty):
    """sum_t log_softmax(logits / T)[seq[t]] over the hypothesis, / len ** length_penalty, in fp64 from the model's own
    logits (forward_infer).  Token t is scored from the last position of the prefix seq[:t] alone: under the inverted
    mask a longer input changes the earlier positions, so one pass over the whole sequence would not be what the steps
    saw."""
    out = []
    for i in range(seqs.shape[0]):
        n = int(lens[i])
        b = i // R
        total = 0.0
        for t in range(1, n + 1):
            dec = seqs[i:i + 1, :t].to(model.device)
            z = model.forward_infer(feats[b:b + 1], decoder_input_ids=dec)["logits"][0, -1].double() / T
            total += float(torch.log_softmax(z, -1)[int(seqs[i, t])])
        out.append(total / n ** length_penalty)
    return out


def _rule_on_oracle(O, ocfg, params, enc, B, K, L, T, lpen):
    """The rule of tests/_beam_ref.py driven by the oracle's fp64 logits; also whether every decision it took had a clear
    margin: each item's order of its 2K + 1 best candidate scores (the order and the 2K boundary) at every step, and the
    stop test.  ``tol`` scales with the logits: the fp32 model's log-probabilities differ from the oracle's by a few 1e-7
    of max |z| / T."""
    lm = params["lm_head.kernel"]
    clear, gaps = True, []

    def lp_fn(prefixes):
        ids = torch.tensor(prefixes, dtype=torch.int64)
        h = O.decoder(params, ids, enc.repeat_interleave(K, 0), ocfg, training=False)
        z = (h[:, -1] @ lm)[:, :V] / T
        return torch.log_softmax(z, -1).numpy(), float(z.abs().max())

    ref = BR.BeamRef(B, K, 1 + L, ocfg.decoder_start_token_id, ocfg.eos_token_id, lpen, False, np.float64)
    for _ in range(L):
        lp, zmax = lp_fn(ref.prefix)
        tol = 1e-5 * zmax
        top = np.sort(lp, 1)[:, ::-1][:, :2 * K + 1]
        for b in range(B):
            if ref.done[b]:
                continue
            sc = np.sort(np.concatenate([ref.sums[b * K + k] + top[b * K + k] for k in range(K)]))[::-1]
            sc = sc[np.isfinite(sc)][:2 * K + 1]
            gaps.append(float((-np.diff(sc)).min()) / tol)
        ids, lps = BR.top_candidates(lp, 2 * K)
        ref.step(ids, lps)
        for b in range(B):
            if len(ref.pools[b]) == K and not ref.done[b]:
                best = max(ref.sums[b * K:(b + 1) * K]) / BR.len_pow(ref.t, lpen, np.float64)
                gaps.append(abs(ref.pools[b][-1][0] - best) / tol)
        if ref.n_done == B:
            break
    ref.finalize()
    clear = min(gaps) > 1.0
    return ref, clear, min(gaps)


def test_generate_beam_matches_reference_rule(dev):
    """Ids and scores of generate(num_beams=3, num_return_sequences=2) against the rule on the oracle's fp64 logits.  With
    the model's own random LM head the top log-probabilities of 51865 columns lie within a few 1e-6 of each other, closer
    than fp32 can order them; the head scaled by 100 spreads them (the smallest gap is then hundreds of times the bound),
    so the comparison is decided by the rule, not by rounding - and it must run."""
    _, whisper, O = _mods()
    ocfg, params, feats, enc = _setup(3000)
    B, K, R, L, T, lpen = feats.shape[0], 3, 2, 10, 0.9, 1.0
    sharp = dict(params)
    sharp["lm_head.kernel"] = params["lm_head.kernel"] * 100.0
    ref, clear, margin = _rule_on_oracle(O, ocfg, sharp, enc, B, K, L, T, lpen)
    assert clear, f"a selection of the fp64 rule is closer than its bound ({margin:.3g} x): the comparison would not decide"
    ref_seq = ref.padded(R, ocfg.pad_token_id)
    _, ref_scores, ref_lens = ref.output(R)
    # the sharpened model is compared with the rule; the model's own head (fp32 and bf16) with its teacher-forced scores
    for precision, p, bound, exact in (("fp32", sharp, 3e-6, True), ("fp32", params, 2e-7, False),
                                       ("bf16", params, 8e-5, False)):
        model = _model(dev, precision, p)
        out = model.generate(feats.to(dev), max_length=L, num_beams=K, num_return_sequences=R, temperature=T,
                             length_penalty=lpen, return_dict_in_generate=True)
        seq, scores, lens = out["sequences"].cpu(), out["sequences_scores"].cpu(), out["lengths"].cpu()
        assert seq.dtype == torch.int32 and seq.shape[0] == B * R and bool((seq[:, 0] == 50257).all())
        assert scores.dtype == torch.float32 and bool(torch.isfinite(scores).all())
        for b in range(B):
            assert bool((scores[b * R:(b + 1) * R].diff() <= 0).all())
        for i in range(B * R):
            assert bool((seq[i, 1 + int(lens[i]):] == ocfg.pad_token_id).all())
        tag = f"{precision}{' x100' if exact else ''}"
        if exact:
            assert torch.equal(seq.long(), torch.from_numpy(ref_seq)), (seq, ref_seq)
            assert lens.tolist() == ref_lens
            for a, r in zip(scores.tolist(), ref_scores):
                within("beam fp32 x100 |score - fp64 rule| / max(1, |score|)", abs(a - r) / max(1.0, abs(r)), 3e-6)
        teacher = _teacher_scores(model, feats.to(dev), seq, lens, R, T, lpen)
        for a, tf in zip(scores.tolist(), teacher):
            within(f"beam {tag} |score - teacher-forced| / max(1, |score|)", abs(a - tf) / max(1.0, abs(tf)), bound)
        assert torch.equal(model.generate(feats.to(dev), max_length=L, num_beams=K, num_return_sequences=R,
                                          temperature=T, length_penalty=lpen), seq.to(dev)), "two calls differ"


def test_generate_num_beams_one_is_greedy_and_eos_paths(dev):
    _, whisper, O = _mods()
    ocfg, params, feats, _ = _setup(3000)
    f = feats[:, :, :800].contiguous().to(dev)
    model = _model(dev, "fp32", params)
    g = model.generate(f, max_length=12)
    assert torch.equal(model.generate(f, max_length=12, num_beams=1), g)
    assert torch.equal(model.generate(f, max_length=12, num_beams=None), g)
    # an EOS column that dominates every row: EOS is every beam's best token, so every hypothesis ends in EOS
    p2 = dict(params)
    p2["decoder.layer_norm.beta"] = torch.full_like(params["decoder.layer_norm.beta"], 10.0)
    lm = params["lm_head.kernel"].clone()
    lm[:, 2] = 1.0
    p2["lm_head.kernel"] = lm
    m2 = _model(dev, "fp32", p2)
    out = m2.generate(f, max_length=20, num_beams=3, num_return_sequences=3, return_dict_in_generate=True,
                      early_stopping=True)
    # (step 1 offers only beam 0's [start, EOS]; the pool fills with later EOS offers, of length 2 or more)
    seq = out["sequences"].cpu()
    assert seq.shape[0] == 6 and bool((seq[:, 0] == 50257).all())
    assert all(int(seq[i, int(out["lengths"][i])]) == 2 for i in range(6))
    # disabled EOS: every hypothesis runs to max_length
    out = model.generate(f, max_length=6, num_beams=4, num_return_sequences=4, eos_token_id=-1, return_dict_in_generate=True)
    assert out["lengths"].tolist() == [6] * 8 and tuple(out["sequences"].shape) == (8, 7)


def _train_run(dev, planned, with_generate, steps=6):
    _, whisper, _ = _mods()
    from tethys_speech_amd import ops, optim, train
    from tethys_speech_amd.data import create_dummy_dataset
    from tethys_speech_amd.dist import DataParallelStrategy
    tiny = dict(d_model=128, encoder_attention_heads=2, decoder_attention_heads=2, d_ff=256, vocab_size=160,
                encoder_layers=2, decoder_layers=2, n_mels=16, n_ctx=64, decoder_start_token_id=150, max_target_positions=32)
    was = ops.set_deterministic(True)
    old = train.USE_PLAN
    try:
        strategy = DataParallelStrategy(0, 1, init=False)
        model = whisper.create_whisper_model("small", device=dev, precision="bf16", seed=5, **tiny)
        model.enable_dropout(0.1, 0.1, seed=77)
        opt = optim.Adam(1e-3)
        it = iter(create_dummy_dataset(3, n_mels=16, seq_len=96, max_target_length=12, device=dev, seed=9, num_samples=8))
        gfeats = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 16, 80)).astype(np.float32)).to(dev)
        train.USE_PLAN = planned
        step = train.planned_step(strategy, model, opt, "whisper", pipelined=True)
        losses, gens = [], []
        for _ in range(steps):
            losses.append(step(*next(it)))
            if with_generate:
                before = model._drop_step
                gens.append(model.generate(gfeats, max_length=5, num_beams=3, num_return_sequences=2).cpu())
                assert model._drop_step == before
        model.finish_late()
        torch.cuda.synchronize()
        return [float(x.item()) for x in losses], model.arena.p.clone(), model.arena.m.clone(), gens
    finally:
        train.USE_PLAN = old
        ops.set_deterministic(was)


@pytest.mark.parametrize("planned", [False, True])
def test_beam_generate_between_training_steps_changes_nothing(dev, planned):
    l0, p0, m0, _ = _train_run(dev, planned, False)
    l1, p1, m1, gens = _train_run(dev, planned, True)
    assert l0 == l1, (l0, l1)
    assert torch.equal(p0, p1) and torch.equal(m0, m1)
    assert len(gens) == 6 and all(g.shape[0] == 4 for g in gens)


# ----------------------------------------------------------------------------- 5. transcription and full size
def test_transcribe_audio_with_beams(dev):
    _, whisper, _ = _mods()
    from tethys_speech_amd.frontend import LogMelFrontend
    _, params, _, _ = _setup(3000)
    model = _model(dev, "bf16", params)
    got = whisper.transcribe_audio(model, None, max_length=8, num_beams=5)
    feats = LogMelFrontend(device=dev)(torch.from_numpy(whisper.dummy_waveform()).to(dev))
    ref = model.generate(feats, max_length=8, num_beams=5)[0].cpu().numpy()
    assert isinstance(got, np.ndarray) and np.array_equal(got, ref) and got[0] == 50257
    assert np.array_equal(whisper.transcribe_audio(model, None, max_length=8),
                          model.generate(feats, max_length=8)[0].cpu().numpy())


def test_full_size_beam_generate_448_steps(dev):
    _, whisper, _ = _mods()
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(8, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    out = model.generate(feats, max_length=448, num_beams=5, num_return_sequences=5, eos_token_id=-1,
                         return_dict_in_generate=True)
    seq, scores, lens = out["sequences"], out["sequences_scores"], out["lengths"]
    assert tuple(seq.shape) == (40, 449) and seq.dtype == torch.int32
    assert bool((seq[:, 0] == 50257).all()) and bool(((seq >= 0) & (seq < V)).all())
    assert bool((lens == 448).all()) and bool(torch.isfinite(scores).all())
    assert bool((scores.view(8, 5).diff(dim=1) <= 0).all())
