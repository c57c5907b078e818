"""CPU: ir-fp (the question injected at g layer 2) on grids with n % 32 != 0 -- the chain predicate on the padded j axis, what
"auto" resolves to, and the oracle against the fixtures recorded from the reference (tests/golden/make_golden_ir_padded.py)."""
import pytest

import gold
from oracle import formula, rn_oracle as O

IR_PADDED_TAGS = ["G-ir196-b32", "G-ir196-small"]
TOL = 2e-5


@pytest.fixture(scope="module")
def pkg():
    import relationnetworks_clevr_amd as p
    return p


def ir_plan(RF, p=2, width=256):
    return RF.LayerPlan(26, 128, [width] * 4, p)


@pytest.mark.parametrize("n,B", [(36, 1), (68, 2), (100, 2), (144, 1), (196, 2), (196, 32), (324, 2), (64, 1)])
def test_chain_covers_ir_fp_on_the_padded_j_axis(pkg, n, B):
    RF = pkg.functional
    assert RF.chain_ok(ir_plan(RF), B, n)


def test_chain_refuses_what_the_padded_ir_fp_chain_does_not_cover(pkg):
    RF = pkg.functional
    assert not RF.chain_ok(ir_plan(RF), 1, 196)          # (B * 196 * 224 % 256 != 0 for odd B: no whole tiles)
    assert not RF.chain_ok(ir_plan(RF), 33, 196)
    assert not RF.chain_ok(ir_plan(RF), 2, 198)          # (n % 4 != 0)
    assert not RF.chain_ok(ir_plan(RF), 4, 10)
    assert not RF.chain_ok(ir_plan(RF), 2, 4)           # (a question shorter than 4 tiles: the dithered roundings do not average out)
    assert not RF.chain_ok(ir_plan(RF), 4, 16)
    assert not RF.chain_ok(ir_plan(RF, width=512), 32, 196)
    for p in (1, 3):                                     # (positions 1 and 3 stay on n % 32 == 0)
        assert not RF.chain_ok(ir_plan(RF, p), 32, 196)
        assert not RF.chain_ok(ir_plan(RF, p), 2, 4)


def test_auto_resolves_to_f16s_for_ir_fp_on_the_stress_grid(pkg):
    hyp = dict(formula.HYP["ir-fp"])
    assert hyp["question_injection_position"] == 2
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], hyp)
    assert rl.precision == "auto"
    assert rl.resolved_precision(32, 196, 26) == "f16s"
    assert rl.resolved_precision(2, 68, 26) == "f16s"
    assert rl.resolved_precision(4, 16, 26) == "fp32"
    assert rl.resolved_precision(1, 196, 26) == "fp32"


@pytest.mark.parametrize("tag", IR_PADDED_TAGS)
def test_oracle_matches_reference_ir_fp_padded(tag):
    g = gold.load(tag)
    meta = g["meta"]
    assert meta["cfg"] == "ir-fp" and meta["n"] % 32 != 0
    hyp, sd, x, q, lab = gold.rl_case(meta)
    params = formula.params_from_state(sd, len(hyp["g_layers"]))
    inj = hyp["question_injection_position"]
    nb = min(meta["b"], 4)                               # (questions are independent: the first four of the big record suffice)
    lp, cache = O.rl_forward_np(x[:nb], q[:nb], params, inj)
    assert gold.rel_err(lp, g["log_probs"][:nb]) <= TOL
    assert gold.rel_err(cache["x_g"], g["x_g"][:nb]) <= TOL
    rows = g["inj_rows"]
    sel = rows < nb * meta["n"] ** 2
    assert sel.sum() >= 4
    assert gold.rel_err(cache["acts"][inj][rows[sel]], g["inj_in_rows"][sel]) <= TOL
    if "dx" in g:                                        # (the full-gradient record)
        dx, dq, gr = O.rl_backward_np(x, q, params, cache, gold.nll_grad(lp, lab))
        assert gold.rel_err(dx, g["dx"]) <= 5 * TOL
        assert gold.rel_err(dq, g["dq"]) <= 5 * TOL
