"""CPU: the error bounds of tests/seqnorm_ref.py are neither loose nor tight by accident. For every
bound and every row count of the contract (seqnorm_ref.L_LIST):

* the fp32 numpy model of the kernels' summation order stays within HALF the bound. Two terms of
  the bounds are a single rounding that reaches its worst case whatever the order, so no model can
  stay under half of them: the bf16 store (2^-8 |v|, met by a value just above a power of two)
  and the fp32 addition of addend (u |addend| where the gradient beside it is small). There the
  half is asked of what the kernel accumulates — y and dx before the bf16 store, dx without
  addend — and the whole bound of the stored value;
* each mutant of the model exceeds the bound by at least 4x somewhere: the last row counted twice,
  the last row dropped, the division by 32 RPT instead of L and, for the backward, a
  register-resident form whose clamped rows' dy is not zeroed.

Where a mutant cannot change a value there is nothing to exceed, and the case is left out by rule,
not by result: the division mutant where 32 RPT = L or the form is two-pass, and for the sums that
are never divided (dgamma, dbeta, the column sums); the unmasked mutant where no row is clamped
(32 RPT = L); at L = 1 the variance is 0 with the row counted once, twice or not at all (rstd is
unchanged) and x - mean = 0 makes every dy * xhat term of dgamma 0."""
import numpy as np
import pytest

from tests import seqnorm_ref as S

B, D = 2, 24
HALF, FOUR = 0.5, 4.0


def _rpt(L):
    """The form by row count alone (the environment switch does not change the model)."""
    return next((r for r in (4, 6, 8, 10) if L <= 32 * r), 0)


def _inputs(L, x_bf16=False):
    g = np.random.default_rng(1000 + L)
    x = (g.standard_normal((B, L, D)) * 2 + 0.5).astype(np.float32)
    add = g.standard_normal((B, L, D)).astype(np.float32)
    if x_bf16:
        x, add = S.bf16_round(x), S.bf16_round(add)
    gamma = g.standard_normal(D).astype(np.float32)
    beta = g.standard_normal(D).astype(np.float32)
    dy = S.bf16_round(g.standard_normal((B, L, D)).astype(np.float32))
    dg0, db0 = (g.standard_normal(D).astype(np.float32) for _ in range(2))
    return x, gamma, beta, dy, add, dg0, db0


def _mutants(L, backward):
    """(name, model arguments, quantities it cannot change)."""
    rpt = _rpt(L)
    never_divided = {"dgamma", "dbeta"}
    at_one = ({"dgamma"} if backward else {"rstd"}) if L == 1 else set()
    out = [("last row twice", {"n_rows": L + 1}, at_one), ("last row dropped", {"n_rows": L - 1}, at_one)]
    if rpt and 32 * rpt != L:
        out.append(("divide by 32 RPT", {"div": 32 * rpt}, never_divided))
        if backward:
            out.append(("clamped dy not zeroed", {"n_rows": 32 * rpt}, at_one))
    return out


@pytest.mark.parametrize("L", S.L_LIST)
def test_forward_bounds_hold_for_the_model_and_catch_the_mutants(L):
    x, gamma, beta, *_ = _inputs(L)
    ref = S.fwd_ref(x, gamma, beta)

    def ratios(**kw):
        mean, rstd, y32, y = S.model_fwd(x, gamma, beta, **kw)
        return {"mean": S.ratio(mean, ref["mean"], ref["mean_bound"]),
                "rstd": S.ratio(rstd, ref["rstd"], ref["rstd_bound"], relative=True),
                "y_f32": S.ratio(y32, ref["y"], ref["y_f32_bound"]),
                "y": S.ratio(y, ref["y"], ref["y_bound"])}

    r = ratios()
    assert r["mean"] <= HALF and r["rstd"] <= HALF and r["y_f32"] <= HALF and r["y"] <= 1.0, r
    for name, kw, unchanged in _mutants(L, backward=False):
        m = ratios(**kw)
        for q in ("mean", "rstd", "y"):
            if q not in unchanged:
                assert m[q] >= FOUR, (name, q, m)


@pytest.mark.parametrize("x_bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", S.L_LIST)
def test_backward_bounds_hold_for_the_model_and_catch_the_mutants(L, x_bf16):
    x, gamma, beta, dy, add, dg0, db0 = _inputs(L, x_bf16)
    mean, rstd, _, _ = S.model_fwd(x, gamma, beta)
    ref = S.bwd_ref(dy, x, mean, rstd, gamma, add, dg0, db0, x_bf16=x_bf16)

    def ratios(**kw):
        dx32, dx, dgam, dbet = S.model_bwd(dy, x, mean, rstd, gamma, add, dg0, db0, x_bf16=x_bf16, **kw)
        return {"dx_f32": S.ratio(dx32, ref["dx"], ref["dx_f32_bound"]),
                "dx": S.ratio(dx, ref["dx"], ref["dx_bound"]),
                "dgamma": S.ratio(dgam, ref["dgamma"], ref["dgamma_bound"]),
                "dbeta": S.ratio(dbet, ref["dbeta"], ref["dbeta_bound"])}

    # what the kernel accumulates, held to half: dx without addend and before a bf16 store
    bare = S.bwd_ref(dy, x, mean, rstd, gamma, None, dg0, db0)
    dx32, _, dgam, dbet = S.model_bwd(dy, x, mean, rstd, gamma, None, dg0, db0)
    assert S.ratio(dx32, bare["dx"], bare["dx_f32_bound"]) <= HALF
    assert S.ratio(dgam, bare["dgamma"], bare["dgamma_bound"]) <= HALF
    assert S.ratio(dbet, bare["dbeta"], bare["dbeta_bound"]) <= HALF
    # with addend (and the bf16 store) the last rounding alone can use all of its term
    r = ratios()
    assert r["dx_f32"] <= 1.0 and r["dx"] <= 1.0 and r["dgamma"] <= HALF and r["dbeta"] <= HALF, r
    for name, kw, unchanged in _mutants(L, backward=True):
        m = ratios(**kw)
        for q in ("dx", "dgamma", "dbeta"):
            if q not in unchanged:
                assert m[q] >= FOUR, (name, q, m)


@pytest.mark.parametrize("L", S.L_LIST)
def test_column_sum_bounds_hold_for_the_model_and_catch_the_mutants(L):
    """The fused dropout backward's column sums: f = dx / keep_prob where kept (here: a fixed
    pattern), z its bf16 rounding. The bound against the sum of f is the one with teeth; the one
    against the sum of z carries the 2^-8 sum|z| of the roundings the kernel does not sum."""
    g = np.random.default_rng(2000 + L)
    dx = g.standard_normal((B, L, D)).astype(np.float32)
    keep = g.random((B, L, D)) < 0.9
    f = np.where(keep, dx * np.float32(1.0 / 0.9), np.float32(0)).astype(np.float32)
    z = S.bf16_round(f)
    init = g.standard_normal(D).astype(np.float32)
    ref = S.colsum_ref(f, z, init)
    got = S.model_colsum(f, init)
    assert S.ratio(got, ref["sum_f"], ref["sum_f_bound"]) <= HALF
    assert S.ratio(got, ref["sum_z"], ref["sum_z_bound"]) <= 1.0
    for n_rows in (L + 1, L - 1):
        assert S.ratio(S.model_colsum(f, init, n_rows), ref["sum_f"], ref["sum_f_bound"]) >= FOUR, n_rows


def test_expected_rpt_states_the_dispatch(monkeypatch):
    monkeypatch.delenv("MMT_SNB_RPT", raising=False)
    want = {1: 4, 128: 4, 129: 6, 192: 6, 193: 8, 256: 8, 257: 10, 320: 10, 321: 0, 512: 0}
    assert {L: S.expected_rpt(L) for L in want} == want
    assert S.expected_rpt(128, x_bf16=True) == 0 and S.expected_rpt(128, dy_bf16=False) == 0
    monkeypatch.setenv("MMT_SNB_RPT", "0")
    assert S.expected_rpt(128) == 0
    monkeypatch.setenv("MMT_SNB_RPT", "1")
    assert S.expected_rpt(128) == 4
