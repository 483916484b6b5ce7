"""fp64 oracle, error bounds and shared cases of the top-k ranking tests (tests/test_topk.py on the CPU,
tests/test_topk_gpu.py on the GPU).

score*(q, c) = qb[q] + cb[c] + <Q[q], C[c]> in fp64, ordered by ``np.lexsort((c, -s))``: greater score first,
equal scores by ascending candidate.  The kernel computes ``((qb + cb) + fmaf chain) + 0`` in fp32: Kp + 2
roundings in a chain, so |s - s*| <= gamma_{Kp+3} (|qb| + |cb| + sum_f |Q_f C_f|) with gamma_n = n u / (1 - n u),
u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; one spare rounding)."""

import numpy as np
import torch

from fast_tffm_amd.ops import kernels as K

U = 2.0 ** -24

KPS = [4, 8, 12, 64, 100, 128, 256]
NQS = [1, 15, 16, 17, 33]
KS = [1, 2, 10, 64, 128]


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def scores64(Q, qb, C, cb) -> np.ndarray:
    Q, qb, C, cb = (np.asarray(t, dtype=np.float64) for t in (Q, qb, C, cb))
    return qb[:, None] + cb[None, :] + Q @ C.T


def tol64(Q, qb, C, cb) -> np.ndarray:
    Q, qb, C, cb = (np.abs(np.asarray(t, dtype=np.float64)) for t in (Q, qb, C, cb))
    return gamma(Q.shape[1] + 3) * (qb[:, None] + cb[None, :] + Q @ C.T)


def oracle_topk(S: np.ndarray, k: int):
    """(idx [nq, k] int32, score [nq, k] fp64) of a score matrix; -1 / -inf past the candidate count."""
    nq, nc = S.shape
    idx = np.full((nq, k), -1, dtype=np.int32)
    score = np.full((nq, k), -np.inf)
    cand = np.arange(nc)
    for q in range(nq):
        order = np.lexsort((cand, -S[q]))[:k]
        idx[q, : order.size] = order
        score[q, : order.size] = S[q, order]
    return idx, score


def slab_of(nq: int, k: int) -> int:
    """The slab length of a small call (every nc up to 4 slabs): from the kernel's own plan."""
    slab, parts = K.topk_plan(nq, 1000, k)
    assert parts == -(-1000 // slab)
    return slab


def ncs(slab: int) -> list[int]:
    return [1, 15, 16, 17, 255, slab - 1, slab, slab + 1, 3 * slab + 5]


def exact_inputs(nq, nc, Kp, seed):
    """Integer profiles in [-4, 4], bases multiples of 0.25 in [-8, 8]: every partial sum is exact in fp32."""
    g = torch.Generator().manual_seed(seed)
    Q = torch.randint(-4, 5, (nq, Kp), generator=g).float()
    C = torch.randint(-4, 5, (nc, Kp), generator=g).float()
    qb = torch.randint(-32, 33, (nq,), generator=g).float() / 4
    cb = torch.randint(-32, 33, (nc,), generator=g).float() / 4
    return Q, qb, C, cb


def run(Q, qb, C, cb, k, device, **kw):
    idx, score = K.fm_topk(Q.to(device), qb.to(device), C.to(device), cb.to(device), k, **kw)
    assert idx.dtype == torch.int32 and score.dtype == torch.float32
    assert tuple(idx.shape) == (Q.shape[0], k) == tuple(score.shape)
    return idx.cpu().numpy(), score.cpu().numpy()


def assert_exact(idx, score, Q, qb, C, cb, k, what=""):
    """Bit for bit the oracle (inputs whose sums are exact in fp32); zeros are +0."""
    want_i, want_s = oracle_topk(scores64(Q, qb, C, cb), k)
    assert np.array_equal(idx, want_i), f"{what}: idx differs from the oracle"
    assert np.array_equal(score.astype(np.float64), want_s), f"{what}: score differs from the oracle"
    assert not np.signbit(score[score == 0]).any(), f"{what}: a -0 score"


def exact_grid_cases(i_kp: int):
    """The pruned product for KPS[i_kp]: the (nq, nc, k) triples whose position indices add up, with
    i_kp, to a multiple of 5 -- every pair of values of two axes occurs together for every Kp."""
    out = []
    for i_q, nq in enumerate(NQS):
        for i_k, k in enumerate(KS):
            slab = slab_of(nq, k)
            for i_c, nc in enumerate(ncs(slab)):
                if (i_kp + i_q + i_k + i_c) % 5 == 0:
                    out.append((nq, nc, k))
    return out


def check_exact_grid(i_kp: int, device):
    Kp = KPS[i_kp]
    cases = exact_grid_cases(i_kp)
    assert len(cases) >= 40
    for n, (nq, nc, k) in enumerate(cases):
        Q, qb, C, cb = exact_inputs(nq, nc, Kp, seed=1000 * i_kp + n)
        idx, score = run(Q, qb, C, cb, k, device)
        assert_exact(idx, score, Q, qb, C, cb, k, what=f"Kp={Kp} nq={nq} nc={nc} k={k}")


# ---- placement across slabs ---------------------------------------------------------------------------------
def placement_cases(slab: int, nc: int, k: int):
    """name -> candidate positions given the k (or 1) greatest base scores, best first."""
    assert nc > 3 * slab + k
    return {
        "last_slab": list(range(nc - k, nc)),
        "one_per_slab": [s * slab + 3 for s in range(4)],
        "first": [0],
        "last": [nc - 1],
        "boundary_left": [2 * slab - 1],
        "boundary_right": [2 * slab],
    }


def check_placement(device):
    nq, Kp, k = 3, 8, 10
    slab = slab_of(nq, k)
    nc = 3 * slab + 37
    assert K.topk_plan(nq, nc, k) == (slab, 4)
    g = torch.Generator().manual_seed(7)
    Q = torch.randint(-1, 2, (nq, Kp), generator=g).float()
    C = torch.randint(-1, 2, (nc, Kp), generator=g).float()       # |dot| <= 8
    qb = torch.tensor([0.25, -3.0, 1.5])
    for name, pos in placement_cases(slab, nc, k).items():
        cb = torch.zeros(nc)
        for rank, c in enumerate(pos):
            cb[c] = 1000.0 - 20.0 * rank                           # gaps above any dot product
        idx, score = run(Q, qb, C, cb, k, device)
        assert_exact(idx, score, Q, qb, C, cb, k, what=name)
        assert (idx[:, : len(pos)] == np.array(pos)[None, :]).all(), name
    # all candidates equal: the answer is 0 .. k-1
    idx, score = run(torch.zeros(nq, Kp), qb, C, torch.full((nc,), 2.0), k, device)
    assert (idx == np.arange(k)[None, :]).all()
    assert (score == (qb.numpy() + 2.0)[:, None]).all()


# ---- random fp32 profiles -------------------------------------------------------------------------------------
def random_inputs(nq, nc, Kp, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(nq, Kp, generator=g), torch.randn(nq, generator=g), torch.randn(nc, Kp, generator=g),
            torch.randn(nc, generator=g))


def assert_within_bounds(idx, score, Q, qb, C, cb, k, what=""):
    """Every returned score within tol of the fp64 score of its candidate, the order by (score, candidate),
    and the returned set admissible: min over R of (s* + tol) >= max over the rest of (s* - tol)."""
    S, T = scores64(Q, qb, C, cb), tol64(Q, qb, C, cb)
    nq, nc = S.shape
    n = min(k, nc)
    assert (idx[:, :n] >= 0).all() and (idx[:, :n] < nc).all(), what
    assert (idx[:, n:] == -1).all() and np.isneginf(score[:, n:]).all(), what
    worst = 0.0
    for q in range(nq):
        r = idx[q, :n]
        assert np.unique(r).size == n, f"{what}: a candidate twice"
        err = np.abs(score[q, :n].astype(np.float64) - S[q, r])
        worst = max(worst, float((err / T[q, r]).max()))
        assert (err <= T[q, r]).all(), f"{what}: query {q} score error / tol = {(err / T[q, r]).max()}"
        s = score[q, :n]
        assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (r[:-1] < r[1:]))).all(), f"{what}: order"
        rest = np.ones(nc, dtype=bool)
        rest[r] = False
        if rest.any():
            assert (S[q, r] + T[q, r]).min() >= (S[q, rest] - T[q, rest]).max(), f"{what}: query {q} not admissible"
    print(f"{what}: max score error / tol = {worst:.3f}")


RANDOM_CASES = [(8, 10), (64, 10), (64, 128), (100, 10)]   # (Kp, k)


def random_case(Kp, k):
    nq = 33
    nc = 3 * slab_of(nq, k) + 5
    return random_inputs(nq, nc, Kp, seed=Kp + k)


# ---- the identity against the scorer -------------------------------------------------------------------------
def identity_batches(V: int, seed: int = 3):
    """(contexts, candidates): CSR batches with values, repeated ids inside an example, and ids shared between
    contexts and candidates (both draw from the same 40 ids)."""
    from fast_tffm_amd.data.batch import Batch

    rng = np.random.default_rng(seed)

    def make(B, lo, hi):
        sizes = rng.integers(lo, hi, size=B)
        sizes[0] = 0 if lo == 0 else sizes[0]
        ids = rng.integers(0, 40, size=int(sizes.sum())) * (V // 41)
        vals = rng.normal(size=ids.size).astype(np.float32)
        off = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(sizes, out=off[1:])
        return Batch(torch.zeros(B), torch.from_numpy(off), torch.from_numpy(ids.astype(np.int32)),
                     torch.from_numpy(vals), None, int(off[-1]))

    return make(9, 0, 12), make(21, 1, 6)


def concat_example(bq, q: int, bc, c: int):
    """(ids, vals) of context q followed by candidate c."""
    s0, e0 = int(bq.offsets[q]), int(bq.offsets[q + 1])
    s1, e1 = int(bc.offsets[c]), int(bc.offsets[c + 1])
    return (np.concatenate([bq.ids[s0:e0].numpy(), bc.ids[s1:e1].numpy()]),
            np.concatenate([bq.vals[s0:e0].numpy(), bc.vals[s1:e1].numpy()]))


def concat_batch(bq, bc):
    """Every (context, candidate) pair as one example, context-major."""
    from fast_tffm_amd.data.batch import Batch

    ids, vals, sizes = [], [], []
    for q in range(bq.B):
        for c in range(bc.B):
            i, v = concat_example(bq, q, bc, c)
            ids.append(i)
            vals.append(v)
            sizes.append(i.size)
    off = np.zeros(len(sizes) + 1, dtype=np.int32)
    np.cumsum(sizes, out=off[1:])
    return Batch(torch.zeros(len(sizes)), torch.from_numpy(off), torch.from_numpy(np.concatenate(ids).astype(np.int32)),
                 torch.from_numpy(np.concatenate(vals).astype(np.float32)), None, int(off[-1]))


def score_and_bound(ids, vals, V64, w64, bias: float, Kp: int):
    """(fp64 score, gamma_{2(n+Kp)+8} M) of one example over the table's stored values."""
    x = vals.astype(np.float64)
    rows = V64[ids] * x[:, None]
    lin = x * w64[ids]
    S = rows.sum(0)
    score = bias + lin.sum() + 0.5 * ((S * S).sum() - (rows * rows).sum())
    A = np.abs(rows).sum(0)
    M = abs(bias) + np.abs(lin).sum() + 0.5 * ((A * A).sum() + (rows * rows).sum())
    return score, gamma(2 * (ids.size + Kp) + 8) * M


def check_identity(model, what=""):
    """``recommend``'s score of (q, c) and the forward of the concatenated example are each within the bound
    of the fp64 score of the concatenated example."""
    from explain_oracle import table_f64

    bq, bc = identity_batches(model.cfg.vocabulary_size)
    dev = model.device
    k = bc.B
    idx, score = model.recommend(bq.to(dev), bc.to(dev), k)
    idx, score = idx.cpu().numpy(), score.cpu().numpy()
    fwd = model.predict(concat_batch(bq, bc).to(dev)).cpu().numpy().reshape(bq.B, bc.B)
    V64, w64, _ = table_f64(model.table.v, model.table.w, model.Kp)
    bias = float(model.gbias) if model.gbias is not None else 0.0
    worst_r = worst_f = 0.0
    for q in range(bq.B):
        assert sorted(idx[q].tolist()) == list(range(k)), f"{what}: query {q} does not list every candidate"
        for j in range(k):
            c = int(idx[q, j])
            ids, vals = concat_example(bq, q, bc, c)
            want, bound = score_and_bound(ids, vals, V64, w64, bias, model.Kp)
            er, ef = abs(float(score[q, j]) - want), abs(float(fwd[q, c]) - want)
            worst_r, worst_f = max(worst_r, er / bound), max(worst_f, ef / bound)
            assert er <= bound, f"{what}: recommend ({q}, {c}) error / bound = {er / bound}"
            assert ef <= bound, f"{what}: forward ({q}, {c}) error / bound = {ef / bound}"
    print(f"{what}: max error / bound: recommend {worst_r:.3f}, forward {worst_f:.3f}")


def make_model(dtype, global_bias: bool, device="cpu", K_=10, V=1013, seed=5):
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig

    cfg = FMConfig(vocabulary_size=V, factor_num=K_, init_value_range=0.5, seed=seed, dtype=dtype,
                   global_bias=global_bias, threads=2)
    m = FactorizationMachine(cfg, device=device)
    if global_bias:
        m.gbias.fill_(0.375)
    return m


def exact_model(device, V=211, K_=8):
    """A model whose table holds small integers / quarters: every score is exact in fp32 in any order, so two
    devices must agree bit for bit."""
    m = make_model(torch.float32, True, device=device, K_=K_, V=V)
    g = torch.Generator().manual_seed(9)
    m.table.v.zero_()
    m.table.v[:V, :K_] = torch.randint(-2, 3, (V, K_), generator=g).float().to(device)
    m.table.w[:V] = (torch.randint(-8, 9, (V,), generator=g).float() / 4).to(device)
    m.gbias.fill_(0.5)
    return m


def exact_batches(V=211, seed=4):
    """Contexts and candidates with values in {1, 2, -1} over a model of ``exact_model``."""
    from fast_tffm_amd.data.batch import Batch

    rng = np.random.default_rng(seed)

    def make(B):
        sizes = rng.integers(1, 5, size=B)
        ids = rng.integers(0, V, size=int(sizes.sum()))
        vals = rng.choice(np.array([1.0, 2.0, -1.0], dtype=np.float32), size=ids.size)
        off = np.zeros(B + 1, dtype=np.int32)
        np.cumsum(sizes, out=off[1:])
        return Batch(torch.zeros(B), torch.from_numpy(off), torch.from_numpy(ids.astype(np.int32)),
                     torch.from_numpy(vals), None, int(off[-1]))

    return make(19), make(300)
