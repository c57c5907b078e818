"""CPU: the question injected at g layer 1 or 3 (the reference's --question-injection N) -- the chain predicate, what "auto"
resolves to, the oracle against the fixtures recorded from the reference (tests/golden/make_golden_inject.py), and the entry
point the last position's backward needs."""
import numpy as np
import pytest

import gold
from oracle import formula, rn_oracle as O

INJ_TAGS = ["G-inj1-small", "G-inj1-64", "G-inj3-small", "G-inj3-64"]
TOL = 2e-5


def inj_case(meta):
    """(hyp, state(np), x, q, labels) of a make_golden_inject fixture: its base config with the injection position of `meta`."""
    hyp = dict(formula.HYP[meta["base_cfg"]], question_injection_position=meta["inject"])
    b, n, seed = meta["b"], meta["n"], meta["seed"]
    k, Q = hyp["rl_in_size"] // 2, hyp["lstm_hidden"]
    sd = formula.formula_rl_state(hyp, seed)
    x = formula.formula_objects(b, n, k, seed + 1, from_pixels=not hyp["state_description"])
    q = formula.hash_uniform((b, Q), seed + 2, -1.0, 1.0)
    lab = formula.hash_ints((b,), seed + 3, 0, formula.ADICT)
    return hyp, sd, x, q, lab


@pytest.fixture(scope="module")
def pkg():
    import relationnetworks_clevr_amd as p
    return p


@pytest.mark.parametrize("p", [1, 3])
def test_chain_covers_injection_at_layer(pkg, p):
    RF = pkg.functional
    assert RF.chain_ok(RF.LayerPlan(26, 128, [256] * 4, p), 64, 64)
    assert RF.chain_ok(RF.LayerPlan(26, 128, [256] * 4, p), 2, 64)
    assert not RF.chain_ok(RF.LayerPlan(26, 128, [256] * 4, p), 2, 196)     # (no padded j axis behind layer 0)
    assert not RF.chain_ok(RF.LayerPlan(26, 128, [512] * 4, p), 64, 64)


@pytest.mark.parametrize("p", [1, 3])
def test_auto_resolves_to_f16s_for_injection_at_layer(pkg, p):
    hyp = dict(formula.HYP["ir-fp"], question_injection_position=p)
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], hyp)
    assert rl.precision == "auto"
    assert rl.resolved_precision(64, 64, 26) == "f16s"


@pytest.mark.parametrize("tag", INJ_TAGS)
def test_oracle_matches_reference_with_injection_at(tag):
    g = gold.load(tag)
    meta = g["meta"]
    assert meta["inject"] in (1, 3) and meta["base_cfg"] == "ir-fp"
    hyp, sd, x, q, lab = inj_case(meta)
    params = formula.params_from_state(sd, len(hyp["g_layers"]))
    lp, cache = O.rl_forward_np(x, q, params, meta["inject"])
    assert gold.rel_err(lp, g["log_probs"]) <= TOL
    assert gold.rel_err(cache["x_g"], g["x_g"]) <= TOL
    assert gold.rel_err(cache["acts"][meta["inject"]][g["inj_rows"]], g["inj_in_rows"]) <= TOL
    dx, dq, gr = O.rl_backward_np(x, q, params, cache, gold.nll_grad(lp, lab))
    assert gold.rel_err(dx, g["dx"]) <= 5 * TOL
    assert gold.rel_err(dq, g["dq"]) <= 5 * TOL


def test_library_takes_the_gate_count_form_of_the_question_sums(pkg):
    """The last position's backward needs the per-question gate counts of the forward masks: the mask form of
    rn_blocked_question_sums (ABI 10; the product ABI keeps its entry-point count), bound as rn_hip.mask_question_counts."""
    import ctypes
    H = pkg.rn_hip
    assert H.ABI_VERSION >= 10 and callable(H.mask_question_counts)
    assert H.SIGNATURES["rn_blocked_question_sums"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_void_p]
    lib = H.load()
    assert lib.rn_abi_version() == H.ABI_VERSION
    # argument checks run on the host: neither or both sources, or a row count the lane masks cannot have, are refused
    Rq = ctypes.c_void_p(16)
    assert lib.rn_blocked_question_sums(None, None, None, Rq, 4096, 4096, None) != 0
    assert lib.rn_blocked_question_sums(ctypes.c_void_p(16), ctypes.c_void_p(16), None, Rq, 4096, 4096, None) != 0
    assert lib.rn_blocked_question_sums(None, ctypes.c_void_p(16), None, Rq, 4096, 16, None) != 0
    assert b"rows_per_question" in lib.rn_last_error()
