"""z by forward substitution over the recursion's blocks, alpha from the split nodes' LINV21 tiles
("Recursion").

The bookkeeping is pinned twice: a numpy restatement of k_rhs, the TRSM and LINV21 epilogues,
k_znode and k_alpha on a random SPD matrix with an arbitrary block table (no device), and the
device's alpha, LML and gradient against oracle/gp_oracle.py at the smallest sizes that reach every
shape of the recursion.  Bounds: those tests/test_gpu.py applies to the same quantities (its
`tolerances` for the LML and the gradient, 1e-9 max|alpha| as test_alpha_export_matches_oracle).
Sizes of at most 8 tiles are one block: their results are compared bit for bit with what the
library gave before the blocks existed (tests/golden/alpha_blocks_n*.npz, recorded from that build
on an MI355X; the inputs are stored with them).
"""
import numpy as np
import pytest

from oracle import gp_oracle as O

D = 3
TS = 64


# ---------------------------------------------------------------------------------------------
# the bookkeeping, without a device
# ---------------------------------------------------------------------------------------------
def alpha_by_blocks(K, y, blocks):
    """K^-1 y the way the device forms it.  blocks: [(lo, hi)] in tiles of TS rows, contiguous from
    0.  zp[h] (h = 2 tj, the odd rows stay zero as for the 64-column producers) and ap[ti] are the
    device's partial rows; every sum below runs over the rows the kernels read."""
    n = K.shape[0]
    nt = n // TS
    L = np.linalg.cholesky(K)
    Linv = np.linalg.inv(L)
    zp = np.full((2 * nt, n), np.nan)  # NaN: a row read before it is written shows
    ap = np.full((nt, n), np.nan)
    z = np.full(n, np.nan)
    alpha = np.empty(n)
    blk_hi = np.empty(nt, dtype=int)

    def rows(t):
        return slice(TS * t, TS * (t + 1))

    for lo, hi in blocks:
        blk_hi[lo:hi] = hi
        # TRSM epilogues of the split ancestors (step 3): every L21 tile left of the block, with the
        # z of its column tile, final by now
        for ti in range(lo, hi):
            for tj in range(lo):
                zp[2 * tj, rows(ti)] = -L[rows(ti), rows(tj)] @ z[rows(tj)]
                zp[2 * tj + 1, rows(ti)] = 0.0
        # k_rhs (step 2)
        Yw = np.array([y[r] + zp[: 2 * lo, r].sum() for r in range(TS * lo, TS * hi)])
        # the block's L^-1 producers: partials of Linv Yw for tj inside the block
        for ti in range(lo, hi):
            for tj in range(lo, ti + 1):
                zp[2 * tj, rows(ti)] = Linv[rows(ti), rows(tj)] @ Yw[TS * (tj - lo):TS * (tj - lo + 1)]
                zp[2 * tj + 1, rows(ti)] = 0.0
        # k_znode (step 4)
        for i in range(lo, hi):
            z[rows(i)] = zp[2 * lo:2 * (i + 1), rows(i)].sum(axis=0)
        # LINV21 epilogues (step 5) of the split nodes that close with this block: all tiles
        # (ti, tj) with ti in the block and tj left of it
        for ti in range(lo, hi):
            for tj in range(lo):
                ap[ti, rows(tj)] = Linv[rows(ti), rows(tj)].T @ z[rows(ti)]
    # k_alpha (step 6)
    Mt = Linv.T
    for i in range(nt):
        k1 = TS * blk_hi[i]
        alpha[rows(i)] = Mt[rows(i), TS * i:k1] @ z[TS * i:k1] + ap[blk_hi[i]:, rows(i)].sum(axis=0)
    return alpha


@pytest.mark.parametrize("sizes", [[3], [2, 2], [1, 3, 2], [4, 5, 4, 5], [2, 1, 1, 3]])
def test_block_bookkeeping_equals_a_solve(sizes):
    nt = sum(sizes)
    n = TS * nt
    rng = np.random.default_rng(nt)
    A = rng.standard_normal((n, n))
    K = A @ A.T / n + np.eye(n)
    y = rng.standard_normal(n)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    got = alpha_by_blocks(K, y, list(zip(edges[:-1], edges[1:])))
    want = np.linalg.solve(K, y)
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))


def blocks_of(nt):
    """factor_rec's splitting rule: a node of more than 8 tiles is halved (top half n // 2)."""
    def rec(o, n):
        return [(o, o + n)] if n <= 8 else rec(o, n // 2) + rec(o + n // 2, n - n // 2)

    return rec(0, nt)


def test_splitting_rule_of_the_test_shapes():
    assert blocks_of(16) == [(0, 8), (8, 16)]
    assert [hi - lo for lo, hi in blocks_of(18)] == [4, 5, 4, 5]
    assert [hi - lo for lo, hi in blocks_of(24)] == [6, 6, 6, 6]
    assert [hi - lo for lo, hi in blocks_of(32)] == [8, 8, 8, 8]
    assert blocks_of(8) == [(0, 8)]


# ---------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------
def make_inputs(N, B, seed=0):
    """As test_input_dimension_extremes: random points, a smooth target plus noise; d = 3."""
    rng = np.random.default_rng(1000 * N + B + seed)
    X = rng.standard_normal((B, D, N))
    Y = np.stack([np.sin(X[s].sum(axis=0)) + 0.05 * rng.standard_normal(N) for s in range(B)])
    T = np.stack([np.concatenate([[-2.0], np.log(np.full(D, 1.5 * np.sqrt(D)) * (1 + 0.1 * rng.random(D))), [0.1]])
                  for _ in range(B)])
    return X, Y, T


@pytest.fixture(scope="module")
def gprx():
    import gprx as g

    return g


@pytest.fixture(scope="module")
def ctx(gprx):
    c = gprx.Context(0)
    yield c
    c.close()


def evaluate(gprx, ctx, X, Y, T):
    b = gprx.GPBatch(Y.shape[0], D, Y.shape[1], 0, ctx=ctx)
    b.set_train(X, Y)
    r = b.run(T, grad=True)
    out = dict(status=r["status"].copy(), mll=r["mll"].copy(), grad=r["grad"].copy(), alpha=b.alpha().copy())
    return b, out


def check_against_oracle(r, s, X, y, theta, mode):
    from test_gpu import tolerances

    f = O.fit(X, y, theta, None, mode)
    t = tolerances(f, O.fit(X, y, theta, None, 1 - mode), y, theta, strict=True)
    da = np.max(np.abs(r["alpha"][s] - f["alpha"]))
    print(f"slot {s}: |d mll| {abs(r['mll'][s] - f['mll']):.3e} (<= {t['mll']:.3e})  "
          f"|d grad| {np.max(np.abs(r['grad'][s] - f['grad'])):.3e} (<= {t['grad']:.3e})  "
          f"|d alpha| {da:.3e} (<= {1e-9 * np.max(np.abs(f['alpha'])):.3e})")
    assert r["status"][s] == 0
    assert abs(r["mll"][s] - f["mll"]) <= t["mll"]
    assert np.max(np.abs(r["grad"][s] - f["grad"])) <= t["grad"]
    assert da <= 1e-9 * np.max(np.abs(f["alpha"]))


@pytest.mark.gpu
@pytest.mark.parametrize("N,B,slots", [
    (1024, 32, (0, 17, 31)),  # one split node over two k_node8 blocks
    (1100, 32, (0, 17, 31)),  # 18 tiles: 9 + 9, blocks of 4, 5, 4, 5 tiles; padded last tile
    (1536, 4, (0, 3)),        # 24 tiles, small batch: 6-tile blocks by k_diag_f, the pair GEMMs, zp_acc2
    (2048, 32, (5, 31)),      # three split nodes over four k_node8 blocks: the bench's recursion
])
def test_split_nodes_against_the_oracle(gprx, ctx, N, B, slots):
    X, Y, T = make_inputs(N, B)
    b, r = evaluate(gprx, ctx, X, Y, T)
    b.close()
    assert np.all(r["status"] == 0)
    for k in ("mll", "grad", "alpha"):
        assert np.all(np.isfinite(r[k])), k
    for s in slots:
        check_against_oracle(r, s, X[s], Y[s], T[s], ctx.dist_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("N,B", [(512, 32), (500, 3)])
def test_single_block_sizes_bit_identical_to_the_recorded_results(gprx, ctx, golden_dir, N, B):
    """At most 8 tiles: one block, k_rhs copies y, k_znode is the former phase 0 and k_alpha adds
    nothing.  Bit for bit what the build before this change gave (recorded), twice in a row."""
    g = np.load(golden_dir / f"alpha_blocks_n{N}_b{B}.npz")
    X, Y, T = g["X"], g["Y"], g["theta"]
    b, r = evaluate(gprx, ctx, X, Y, T)
    r2 = b.run(T, grad=True)
    a2 = b.alpha()
    b.close()
    for k in ("mll", "grad", "alpha"):
        np.testing.assert_array_equal(r[k].view(np.uint64), g[k].view(np.uint64), err_msg=k)
    np.testing.assert_array_equal(r2["mll"], r["mll"])
    np.testing.assert_array_equal(r2["grad"], r["grad"])
    np.testing.assert_array_equal(a2, r["alpha"])
    check_against_oracle(r, B - 1, X[B - 1], Y[B - 1], T[B - 1], ctx.dist_mode)


@pytest.mark.gpu
def test_no_state_between_evaluations(gprx, ctx):
    """Two evaluations with different theta on one batch equal the same two on fresh batches: Yw,
    ap and zp are rewritten by every evaluation before they are read."""
    N, B = 1100, 32
    X, Y, T = make_inputs(N, B)
    T2 = T + 0.3 * np.random.default_rng(3).standard_normal(T.shape)
    b, r1 = evaluate(gprx, ctx, X, Y, T)
    r2 = b.run(T2, grad=True)
    r2 = dict(mll=r2["mll"].copy(), grad=r2["grad"].copy(), alpha=b.alpha().copy())
    b.close()
    for Tf, got in ((T, r1), (T2, r2)):
        bf, want = evaluate(gprx, ctx, X, Y, Tf)
        bf.close()
        for k in ("mll", "grad", "alpha"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.gpu
def test_masked_optimiser_rounds_match_single_slot_runs(gprx, ctx):
    """As test_device_optimize_ragged_batch_equals_single_slot_runs, at a size with split nodes:
    slots that stop early are masked out of the later rounds (k_rhs, k_znode and k_alpha go
    through map_slot), and every slot's result is bit-identical to optimising it alone."""
    from gprx.optim import LBFGS, Options

    N, B = 1100, 4
    X, Y, T = make_inputs(N, B, seed=1)
    T = T + np.array([0.02, 0.6, 0.1, 0.9])[:, None] * np.random.default_rng(4).standard_normal(T.shape)
    opts = Options(iterations=6)
    b = gprx.GPBatch(B, D, N, 0, ctx=ctx)
    b.set_train(X, Y)
    dev, _ = b.optimize(T, LBFGS(), opts, refit=False)
    b.close()
    assert len({r.f_calls for r in dev}) > 1  # ragged: some rounds ran with slots masked out
    one = gprx.GPBatch(1, D, N, 0, ctx=ctx)
    for s in range(B):
        one.set_train(X[s:s + 1], Y[s:s + 1])
        (r1,), _ = one.optimize(T[s:s + 1], LBFGS(), opts, refit=False)
        assert (r1.iterations, r1.f_calls, r1.g_calls, r1.stopped_by) == (
            dev[s].iterations, dev[s].f_calls, dev[s].g_calls, dev[s].stopped_by), s
        np.testing.assert_array_equal(r1.minimizer, dev[s].minimizer)
        assert r1.minimum == dev[s].minimum
    one.close()
