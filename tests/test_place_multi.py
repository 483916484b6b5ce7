"""Several held-out targets per context: ``ops.kernels.fm_place`` with a target pair, ``place_metrics(offsets=)`` and
``run.py recommend`` with multi-integer target lines -- the CPU twin against fp64 references (the shared cases of
tests/test_place_multi_gpu.py live here)."""

import contextlib
import io
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import place_oracle as PO
from fast_tffm_amd import cli
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.ops import native
from test_topk import CANDS, LINES, _copy_lines, _load, _trainer, _write_cfg
from topk_oracle import exact_inputs, scores64

S = K.PLACE_SEGMENT
CPU = torch.device("cpu")


def target_lists(nq, nc, slab, seed):
    """Context 0 holds S + 1 targets (all of 33 candidates), the others 0, 1, 2, S, S + 1, 2 S + 3 in turn, capped at
    nc: uncapped, context 12's three rows are 15 .. 17 and context 48's 63 .. 65 -- across a 16-row tile and a 64-row
    workgroup.  Candidate 0, the last one, a slab's last and the next slab's first come first in every list."""
    rng = np.random.default_rng(seed)
    special = [t for t in (0, nc - 1, slab - 1, slab) if t < nc]
    lens = [S + 1] + [(0, 1, 2, S, S + 1, 2 * S + 3)[i % 6] for i in range(nq - 1)]
    return [sorted(list(dict.fromkeys(special + rng.permutation(nc).tolist()))[:min(n, nc)]) for n in lens]


def seen_for(S64, lists, seed):
    """Per context: one of its targets (it still competes), a candidate that ties a target, and ordinary ones."""
    rng = np.random.default_rng(seed)
    out = []
    for q, ts in enumerate(lists):
        row = set(rng.integers(0, S64.shape[1], 5).tolist()) | set(ts[:1])
        ties = [c for t in ts[:4] for c in np.flatnonzero(S64[q] == S64[q, t]) if c not in ts]
        out.append(sorted(row | set(ties[:1])))
    return out


def counts64(S64, lists, seen=None):
    out = []
    for q, ts in enumerate(lists):
        comp = np.ones(S64.shape[1], dtype=bool)
        if seen is not None:
            comp[seen[q]] = False
            comp[ts] = True
        out += [((S64[q, comp] > S64[q, t]).sum(), (S64[q, comp] == S64[q, t]).sum()) for t in ts]
    return np.array(out, dtype=np.int32).reshape(-1, 2)


def check_exact(Kp, nq, device, with_seen):
    """counts == the fp64 reference on profiles whose every sum is exact in fp32 (ties abound)."""
    slab = PO.slab_of(nq)
    for nc in (33, slab + 1, 3 * slab + 5):
        Q, qb, C, cb = exact_inputs(nq, nc, Kp, seed=Kp + nq + nc)
        S64 = scores64(Q, qb, C, cb)
        lists = target_lists(nq, nc, slab, seed=nc)
        seen = seen_for(S64, lists, seed=nq) if with_seen else None
        ps = K.fm_place(Q.to(device), qb.to(device), C.to(device), cb.to(device), K.seen_lists(lists, nc, device),
                        PO.CUTOFFS, seen=None if seen is None else K.seen_lists(seen, nc, device))
        got, want = ps.counts().cpu().numpy(), counts64(S64, lists, seen)
        wrong = np.flatnonzero((got != want).any(1))
        w8 = wrong[:8]
        assert wrong.size == 0, f"Kp={Kp} nq={nq} nc={nc}: entries {w8} got {got[w8]} want {want[w8]}"
        assert ps.ranked() == sum(1 for t in lists if t) and ps.entries() == len(want)


def check_single(device):
    """Lists of at most one target: per ranked context the counts of the tensor form."""
    nq, nc = 21, 300
    Q, qb, C, cb = (x.to(device) for x in exact_inputs(nq, nc, 12, seed=5))
    t = PO.targets(nq, nc, PO.slab_of(nq), 0, seed=1)
    seen = K.seen_lists([[int(x) % nc for x in (q, 7 * q, t[q])] for q in range(nq)], nc, device)
    for sn in (None, seen):
        one = K.fm_place(Q, qb, C, cb, t.to(device), seen=sn).counts().cpu()
        pair = K.seen_lists([[x] if x >= 0 else [] for x in t.tolist()], nc, device)
        assert torch.equal(K.fm_place(Q, qb, C, cb, pair, seen=sn).counts().cpu(), one[t >= 0])


# contexts as lists of (greater, equal): tie runs straddling the cutoffs 1 / 5 / 10, more and fewer targets than a
# cutoff, a context without targets, places past every cutoff
METRIC_CONTEXTS = [[(0, 3), (3, 1), (4, 4)], [(8, 5)], [], [(0, 1)], [(g, 1) for g in range(12)], [(9, 2), (30, 1)],
                   [(2, 2), (2, 2), (100, 7)], [(0, 40)] * 40 + [(40, 1)]]


def metrics_ref(ctxs, cutoffs):
    """{(name, k): sum over the ranked contexts} with Fractions and math.fsum."""
    D = [math.fsum(1.0 / math.log2(j + 1.0) for j in range(1, r + 1)) for r in range(max(cutoffs) + 1)]
    out = {}
    for k in cutoffs:
        rec = ndcg = prec = Fraction(0)
        for c in filter(None, ctxs):
            hits = sum(Fraction(min(g + e, k) - min(g, k), e) for g, e in c)
            dcg = math.fsum((D[min(g + e, k)] - D[min(g, k)]) / e for g, e in c)
            rec += hits / len(c)
            prec += hits / k
            ndcg += Fraction(dcg / D[min(len(c), k)])
        out["recall", k], out["ndcg", k], out["precision", k] = float(rec), float(ndcg), float(prec)
    return out


def check_metrics(device):
    rng = np.random.default_rng(0)
    many = [[(int(g), int(e)) for g, e in zip(rng.integers(0, 30, n), rng.integers(1, 4, n))]
            for n in rng.integers(0, 5, 1100)]
    cutoffs = (1, 5, 10)
    for ctxs in (METRIC_CONTEXTS, many, [[], []]):
        off = torch.tensor(np.cumsum([0] + [len(c) for c in ctxs]), dtype=torch.int32, device=device)
        rows = torch.tensor([r for c in ctxs for r in c], dtype=torch.int32, device=device).reshape(-1, 2)
        ps = K.place_metrics(rows, cutoffs, offsets=off)
        ranked, entries = sum(1 for c in ctxs if c), sum(len(c) for c in ctxs)
        assert (ps.ranked(), ps.entries()) == (ranked, entries)
        if not ranked:
            assert math.isnan(ps.recall(5)) and math.isnan(ps.mean_place())
            continue
        assert ps.mean_place() == sum(2 * g + e + 1 for c in ctxs for g, e in c) / (2 * entries)
        # a context's value lies in [0, 1] and takes at most |T| + 2 fp64 operations
        tol = len(ctxs) * (max(len(c) for c in ctxs) + 3) * 2.0 ** -52
        for (name, k), want in metrics_ref(ctxs, cutoffs).items():
            got = getattr(ps, name)(k) * ranked
            print(f"{name}@{k}: sum {got!r} want {want!r} tol {tol:.3g}")
            assert abs(got - want) <= tol, (name, k, got, want)


@pytest.mark.parametrize("with_seen", [False, True])
@pytest.mark.parametrize("nq", PO.EXACT_NQS)
@pytest.mark.parametrize("Kp", PO.EXACT_KPS)
def test_exact_counts(Kp, nq, with_seen):
    check_exact(Kp, nq, CPU, with_seen)


def test_single_target_lists():
    check_single(CPU)


def test_metrics():
    assert S == native.cpu().PLACE_SEGMENT
    check_metrics(CPU)


def test_shortlist_refused():
    Q, qb, C, cb = exact_inputs(2, 9, 4, seed=0)
    pair = K.seen_lists([[1], [2, 3]], 9, CPU)
    with pytest.raises(ValueError, match="shortlist"):
        K.fm_place(Q, qb, C, cb, pair, shortlist=pair)


# ---- run.py recommend ------------------------------------------------------------------------------------------
def _targets_of(i):
    return [] if i == 4 else sorted({(37 * i + 11 * j) % CANDS for j in range(1 + i % 4)})


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, ref_data_dir):
    wd = str(tmp_path_factory.mktemp("place_multi_cli"))
    os.makedirs(os.path.join(wd, "data"))
    _copy_lines(os.path.join(ref_data_dir, "train_0"), os.path.join(wd, "data", "train_0"), 0, 600)
    _copy_lines(os.path.join(ref_data_dir, "test_0"), os.path.join(wd, "data", "test_0"), 0, LINES)
    cands = os.path.join(wd, "data", "candidates")
    _copy_lines(os.path.join(ref_data_dir, "test_0"), cands, LINES, CANDS)
    targets = os.path.join(wd, "data", "targets")
    with open(targets, "w") as f:   # (a duplicate on every line with targets: it collapses)
        f.write("".join(" ".join(map(str, (t := _targets_of(i)) + t[:1])) + "\n" if _targets_of(i) else "-1\n"
                        for i in range(LINES)))
    cfg = os.path.join(wd, "targets.cfg")
    with open(_write_cfg(wd)) as f, open(cfg, "w") as g:
        g.write(f.read().replace("[Distributed]", f"recommend_target_files = {targets}\n\n[Distributed]"))
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["train", cfg, "--max-steps", "4"]) == 0
    return wd, cfg, cands, targets


def test_cli_places(workdir):
    wd, cfg, cands, _ = workdir
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main(["recommend", cfg, "--candidates", cands, "--top", "5"]) == 0
    tr = _trainer(cfg)
    lists = [_targets_of(i) for i in range(LINES)]
    want = tr.model.place(_load(tr, os.path.join(wd, "data", "test_0")), _load(tr, cands),
                          K.seen_lists(lists, CANDS, CPU), (5,)).counts().tolist()
    rows = [list(map(int, ln.split())) for ln in open(os.path.join(wd, "data", "test_0_places"))]
    assert rows[4] == [-1, 0, 0] and len(rows) == LINES
    got = [r[3 * j:3 * j + 3] for i, r in enumerate(rows) if i != 4 for j in range(len(r) // 3)]
    assert got == [[t, gt, eq] for t, (gt, eq) in zip((t for ts in lists for t in ts), want)]
    m = re.search(r"contexts (\d+) ranked (\d+) targets (\d+) recall@5 (\S+) ndcg@5 \S+ precision@5 \S+ mean_place",
                  out.getvalue())
    assert tuple(map(int, m.group(1, 2, 3))) == (LINES, LINES - 1, len(want))
    recall = sum(sum(Fraction(min(gt + eq, 5) - min(gt, 5), eq) for _, gt, eq in
                     (r[3 * j:3 * j + 3] for j in range(len(r) // 3))) / (len(r) // 3)
                 for i, r in enumerate(rows) if i != 4) / (LINES - 1)
    assert float(m.group(4)) == float("%.8f" % float(recall))


def test_cli_malformed_line(workdir):
    _, cfg, cands, targets = workdir
    good = open(targets).read()
    lines = good.splitlines()
    lines[6] = "3 -1 8"   # (-1 is "none" only alone)
    try:
        with open(targets, "w") as f:
            f.write("\n".join(lines) + "\n")
        with pytest.raises(ValueError, match=re.escape(targets) + ", line 7:"), \
                contextlib.redirect_stdout(io.StringIO()):
            cli.main(["recommend", cfg, "--candidates", cands, "--top", "5"])
    finally:
        with open(targets, "w") as f:
            f.write(good)
