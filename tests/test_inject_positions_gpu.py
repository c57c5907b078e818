"""GPU: the question injected at g layer 1 or 3 on the register-resident chains (f16s): the forward kernel's new variants against
the float64 emulation of their arithmetic, the per-question gate counts of the last layer, parity with the reference's fixtures
(tests/golden/make_golden_inject.py) in every mode that accepts the shapes, both sources of the injected layer's question sums,
the question gradient handed over by event, the batch-independent eval arithmetic, and the graph-replayed trainer."""
import numpy as np
import pytest
import torch

import gold
from oracle import formula
from test_gpu_kernels import (F16S_V, check_against_f16s_emulation, dev, dither_images, f16s_images, gate_image_ref, rr_mask_decode,
                              unblock, unblock_h)
from test_gpu_parity import CONTRACT, F16S_GUARD, l2rel, report
from test_inject_positions_cpu import INJ_TAGS, inj_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    import relationnetworks_clevr_amd as pkg
    pkg.rn_hip.load()
    torch.cuda.set_device(0)
    return pkg.rn_hip


@pytest.fixture(scope="module")
def pkg():
    import relationnetworks_clevr_amd as p
    p.rn_hip.load()
    torch.cuda.set_device(0)
    return p


def inj_emulation(x, Vq, Ws, bs, n, inj):
    """float64 emulation of the f16s chain with the question at layer inj > 0: layer 0 factored without the question (tables built
    with Q = 0), layers 1..3 the fp16-rounded previous activation @ the tile's dithered hi image of W_l[:, 0:256], the injected layer's
    bias the per-question row Vq[b] (fp32, as the kernel reads it).  -> (pre-activations, valid rows, the exact chain's last layer)."""
    B, _, k = x.shape
    G, L = 256, len(Ws)
    f16r = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    M = B * n * n
    r = np.arange(M)
    b_of, i_of, j_of = r // (n * n), (r // n) % n, r % n
    xj = x[b_of, j_of]
    W0 = Ws[0].astype(np.float64)
    wh = f16r(Ws[0][:, :k]); wl = f16r(Ws[0][:, :k] - wh)
    brack = x[b_of, i_of].astype(np.float64) @ W0[:, k:2 * k].T + bs[0]
    zs = [f16r(xj).astype(np.float64) @ (wh.astype(np.float64) + wl.astype(np.float64)).T + brack]
    exact = np.maximum(xj.astype(np.float64) @ W0[:, :k].T + brack, 0)
    timg = (r // 256) % F16S_V
    prev = f16r(np.maximum(zs[0], 0)).astype(np.float64)
    for l in range(1, L):
        bias = Vq[b_of].astype(np.float64) if l == inj else np.broadcast_to(bs[l].astype(np.float64), (M, G))
        z = np.empty((M, G))
        for d, im in enumerate(dither_images(Ws[l][:, :G])):
            sel = timg == d
            z[sel] = prev[sel] @ im.astype(np.float64).T + bias[sel]
        zs.append(z)
        exact = np.maximum(exact @ Ws[l][:, :G].astype(np.float64).T + bias, 0)
        prev = f16r(np.maximum(z, 0)).astype(np.float64)
    return zs, np.ones(M, bool), exact


@pytest.mark.parametrize("inj", [1, 3])
def test_g_chain_fwd_rr_f16s_alg0_injected_at(H, inj):
    """rn_g_chain_fwd_rr_f16s_alg0 with inject_layer 1 / 3 (B = 19: 304 tiles, so workgroups carry the next tile's question row
    across questions): 16-bit copies, masks and pair sums against the emulation; the e4m3 copies, then the gate in the sign bits of
    H_2, bitwise against the 16-bit run where they must be; the two inference variants' pair sums against the same emulation."""
    L, G, k, Q, B, n = 4, 256, 26, 128, 19, 64
    M, kt = B * n * n, 2 * k
    x = formula.hash_uniform((B, n, k), 500 + inj, -1, 1).astype(np.float32)
    q = formula.hash_uniform((B, Q), 510 + inj, -1, 1).astype(np.float32)
    Ws = [formula.hash_uniform((G, kt if l == 0 else G + (Q if l == inj else 0)), 520 + l, -0.15, 0.15).astype(np.float32) for l in range(L)]
    bs = [formula.hash_uniform((G,), 530 + l, -0.3, 0.3).astype(np.float32) for l in range(L)]
    Vq = (q.astype(np.float64) @ Ws[inj][:, G:].T.astype(np.float64) + bs[inj]).astype(np.float32)
    wd = [dev(w) for w in Ws]
    w0T = torch.empty(kt, G, device="cuda")
    his, lo0, jobs = f16s_images(H, wd, kt, k)
    jobs = [j if j[0] is not wd[inj] else (wd[inj], G + Q, 1, G, G, his[inj], j[6]) for j in jobs]   # (the H columns of W_inj)
    H.pack_matrix_frag_many(jobs + [(wd[0], kt, 1, G, kt, w0T, 2)])
    Xp = torch.empty(B * n, 64, dtype=torch.float16, device="cuda"); Vc = torch.empty(B * n, G, device="cuda")
    H.pair_tables(dev(x), None, w0T, dev(bs[0]), Xp, Vc, B, n, k, 0, G)
    bd, Vqd = [dev(b) for b in bs], dev(Vq)

    def run(dtype, gate=False):
        if dtype == torch.bfloat16:
            Hs = [torch.full((M, G), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)] + [None]
        else:                                                      # (e4m3: one byte per element, 0x7f = NaN)
            Hs = [torch.full((M, G), 0x7f, dtype=torch.uint8, device="cuda").view(dtype) for _ in range(3)] + [None]
        assert all(h.shape == (M, G) for h in Hs[:3])
        masks = list(torch.zeros(L, H.g_chain_rr_mask_bytes(M), dtype=torch.uint8, device="cuda"))
        part = torch.full((M // 256, G), float("nan"), dtype=torch.float32, device="cuda")
        H.g_chain_fwd_rr_f16s_alg0(Xp, Vc, n, his, lo0, bd, Hs, masks, part, M, G, Vq=Vqd, inject=inj, gate=gate)
        torch.cuda.synchronize()
        return Hs, masks, part

    Hs16, m16, p16 = run(torch.bfloat16)
    Hs16 = unblock_h(Hs16)
    zs, valid, exact = inj_emulation(x, Vq, Ws, bs, n, inj)
    check_against_f16s_emulation(zs, valid, exact, Hs16, m16, p16, M)
    Hs8, m8, p8 = run(torch.float8_e4m3fn)
    Hs8 = unblock_h(Hs8)
    assert torch.equal(p16, p8)
    for l in range(L):
        assert torch.equal(m16[l], m8[l]), l
    for l in range(3):
        ref8 = Hs16[l].float().to(torch.float8_e4m3fn)
        assert (Hs8[l].view(torch.uint8) == ref8.view(torch.uint8)).float().mean().item() >= 0.97, l
        d = (Hs8[l].float() - Hs16[l].float()).abs()
        assert bool((d <= Hs16[l].float().abs() * 2.0 ** -4 + 2.0 ** -10).all()), l
    Hg, mg, pg = run(torch.float8_e4m3fn, gate=True)
    assert torch.equal(pg, p8)
    for l in range(L):
        assert torch.equal(mg[l], m8[l]), l
    for l in range(2):
        assert torch.equal(unblock(Hg[l]).view(torch.uint8), Hs8[l].view(torch.uint8)), l
    assert torch.equal(unblock(Hg[2]).view(torch.uint8) & 0x7f, Hs8[2].view(torch.uint8))
    assert torch.equal(unblock(Hg[2]).view(torch.uint8) >> 7, gate_image_ref(m8[3], M).to(torch.uint8))
    # inference: one pass on the dithered images, and two passes (hi + lo on every layer)
    pi = torch.full((M // 256, G), float("nan"), dtype=torch.float32, device="cuda")
    H.g_chain_fwd_rr_f16s_alg0(Xp, Vc, n, his, lo0, bd, None, None, pi, M, G, Vq=Vqd, inject=inj)
    torch.cuda.synchronize()
    check_against_f16s_emulation(zs, valid, exact, None, None, pi, M)
    his2 = [torch.empty(1, 65536, dtype=torch.float16, device="cuda") for _ in range(L)]
    los2 = [torch.empty(65536, dtype=torch.float16, device="cuda") for _ in range(L)]
    j2 = [(wd[0], kt, 1, G, k, his2[0], 4 | 1), (wd[0], kt, 1, G, k, los2[0], 8 | 1)]
    j2 += [(wd[l], Ws[l].shape[1], 1, G, G, his2[l], 4) for l in range(1, L)] + [(wd[l], Ws[l].shape[1], 1, G, G, los2[l], 8) for l in range(1, L)]
    H.pack_matrix_frag_many(j2)
    p2 = torch.full((M // 256, G), float("nan"), dtype=torch.float32, device="cuda")
    H.g_chain_fwd_rr_f16s_alg0(Xp, Vc, n, his2, los2, bd, None, None, p2, M, G, Vq=Vqd, inject=inj)
    torch.cuda.synchronize()
    last = np.maximum(zs[-1], 0)
    assert l2rel(p2.cpu().numpy(), exact.reshape(M // 256, 256, G).sum(1)) <= 1e-3
    assert l2rel(p16.cpu().numpy(), last.reshape(M // 256, 256, G).sum(1)) <= 1e-3
    # the per-question counts of the last layer's gate (rn_mask_question_counts): exact, and dxg x counts in one fp32 product
    C = torch.from_numpy(rr_mask_decode(m8[3], M, 3).reshape(B, n * n, G).sum(1).astype(np.float32)).cuda()
    got = torch.full((B, G), float("nan"), device="cuda")
    H.mask_question_counts(m8[3], got, M, n * n)
    dxg = torch.from_numpy(formula.hash_uniform((B, G), 540, -1, 1).astype(np.float32)).cuda()
    got_s = torch.full((B, G), float("nan"), device="cuda")
    H.mask_question_counts(m8[3], got_s, M, n * n, dxg=dxg)
    torch.cuda.synchronize()
    assert torch.equal(got, C)
    assert torch.equal(got_s, dxg * C)


def test_mask_question_counts_refuses_bad_shapes(H):
    m = torch.zeros(H.g_chain_rr_mask_bytes(4096), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        H.mask_question_counts(m, torch.empty(2, 256, device="cuda"), 4096, 4096)        # (one question: out must be (1, 256))
    with pytest.raises(RuntimeError):
        H.mask_question_counts(m, torch.empty(256, 256, device="cuda"), 4096, 16)         # (rows per question % 32 != 0)


def run_inj(pkg, g, precision):
    meta = g["meta"]
    hyp, sd, x, q, lab = inj_case(meta)
    hyp = dict(hyp, precision=precision)
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], hyp)
    rl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    rl = rl.cuda().eval()
    if meta.get("strided"):
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().permute(0, 2, 1)
    else:
        xt = torch.from_numpy(x).cuda()
    xt.requires_grad_(True)
    qt = torch.from_numpy(q).cuda().requires_grad_(True)
    lp = rl(xt, qt)
    loss = torch.nn.functional.nll_loss(lp, torch.from_numpy(lab).cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {n_: p_.grad.detach().cpu().numpy() for n_, p_ in rl.named_parameters()}
    return lp.detach().cpu().numpy(), float(loss.detach()), xt.grad.cpu().numpy(), qt.grad.cpu().numpy(), grads


@pytest.mark.parametrize("tag", INJ_TAGS)
def test_injected_f16s_parity(pkg, tag):
    """The bars of test_relational_layer_f16s_parity; "auto" resolves to this mode on these shapes."""
    g = gold.load(tag)
    hyp = inj_case(g["meta"])[0]
    assert pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], dict(hyp)).resolved_precision(
        g["meta"]["b"], g["meta"]["n"], hyp["rl_in_size"] // 2) == "f16s"
    lp, loss, dx, dq, grads = run_inj(pkg, g, "f16s")
    e_lp = gold.rel_err(lp, g["log_probs"])
    e_dx, e_dq = l2rel(dx, g["dx"]), l2rel(dq, g["dq"])
    e_b = max(l2rel(grads[k[5:]], g[k]) for k in g if k.startswith("grad/"))
    agree = float((lp.argmax(1) == g["log_probs"].argmax(1)).mean())
    per = {}
    e_w = gold.check_grads(g, grads, 3e-2, per)
    report(tag, precision="f16s", log_probs=e_lp, dx_l2=e_dx, dq_l2=e_dq, params_l2=e_b, argmax_agree=agree, param_grads_max=e_w)
    assert e_lp <= CONTRACT
    assert e_lp <= F16S_GUARD, "regression guard (the contract, 1e-3, still holds)"
    assert agree == 1.0
    assert e_dx <= 2e-2 and e_dq <= 2e-2 and e_b <= 1.2e-2, (e_dx, e_dq, e_b)
    if g["dx"].shape[0] >= 32:
        pq = lambda a, r: np.array([l2rel(a[i], r[i]) for i in range(a.shape[0])])
        mx, mq = float(np.median(pq(dx, g["dx"]))), float(np.median(pq(dq, g["dq"])))
        report(tag, precision="f16s", dx_l2_median_per_question=mx, dq_l2_median_per_question=mq)
        assert mx <= 1.5e-2 and mq <= 6e-3, (mx, mq)


@pytest.mark.parametrize("tag", INJ_TAGS)
def test_injected_fp32_and_bf16x3_parity(pkg, tag):
    g = gold.load(tag)
    lp, loss, dx, dq, grads = run_inj(pkg, g, "fp32")
    e_lp, e_dx, e_dq = gold.rel_err(lp, g["log_probs"]), gold.rel_err(dx, g["dx"]), gold.rel_err(dq, g["dq"])
    e_w = gold.check_grads(g, grads, 1e-3, {})
    report(tag, precision="fp32", log_probs=e_lp, dx=e_dx, dq=e_dq, params=e_w)
    assert e_lp <= 1e-4
    assert abs(loss - float(g["loss"])) <= 1e-4 * max(1.0, abs(float(g["loss"])))
    assert e_dx <= 5e-3 and e_dq <= 5e-3
    # (the per-layer fp32 path's own bar is 2e-4; on G-inj3-small, B = 2, a g_theta unit within fp32 round-off of its ReLU kink gates
    # differently under another summation order and carries dx to 2.6e-4 -- max-norm 9e-4, inside the 5e-3 above)
    assert l2rel(dx, g["dx"]) <= 5e-4 and l2rel(dq, g["dq"]) <= 2e-4
    lp, loss, dx, dq, grads = run_inj(pkg, g, "bf16x3")
    e_lp, e_dx, e_dq = gold.rel_err(lp, g["log_probs"]), l2rel(dx, g["dx"]), l2rel(dq, g["dq"])
    e_b = max(l2rel(grads[k[5:]], g[k]) for k in g if k.startswith("grad/"))
    report(tag, precision="bf16x3", log_probs=e_lp, dx_l2=e_dx, dq_l2=e_dq, params_l2=e_b)
    assert e_lp <= 1e-4 and e_dx <= 1e-3 and e_dq <= 1e-3 and e_b <= 1e-3, (e_lp, e_dx, e_dq, e_b)


@pytest.mark.parametrize("tag", ["G-inj1-64", "G-inj3-64", "G-inj1-small", "G-inj3-small"])
def test_injected_question_sums_from_either_source(pkg, tag, monkeypatch):
    """Rq of the injected layer from the weight-gradient launch's question-aligned db partials, or from a pass of its own (forced by
    hiding the aligned split count): layer 1 -- rn_blocked_question_sums over the stored dZ_1; layer 3 -- dxg x the gate counts of
    the forward masks (rn_mask_question_counts: dZ_3 is never stored).  Forward and dx bitwise, dq and the g-layer gradients to
    1e-5, the rest bitwise."""
    g = gold.load(tag)
    inj = g["meta"]["inject"]
    real = pkg.rn_hip.wgrad_blocked_splits
    monkeypatch.setattr(pkg.rn_hip, "wgrad_blocked_splits", lambda M, rpq=0, njobs=1, aligned=False: 0 if aligned else real(M, rpq, njobs, aligned))
    lp0, loss0, dx0, dq0, gr0 = run_inj(pkg, g, "f16s")
    monkeypatch.setattr(pkg.rn_hip, "wgrad_blocked_splits", real)
    lp1, loss1, dx1, dq1, gr1 = run_inj(pkg, g, "f16s")
    assert np.array_equal(lp0, lp1) and np.array_equal(dx0, dx1)
    report(tag, precision="f16s", rq_sources_dq_l2=l2rel(dq1, dq0))
    assert l2rel(dq1, dq0) <= 1e-5
    for k in gr0:
        if k.startswith("g_layers.") and not k.startswith("g_layers.0."):
            assert l2rel(gr1[k], gr0[k]) <= 1e-5, k
            if k == "g_layers.%d.weight" % inj:
                assert l2rel(gr1[k][:, 256:], gr0[k][:, 256:]) <= 1e-5
        else:
            assert np.array_equal(gr0[k], gr1[k]), k


class Args:
    qdict_size, adict_size = 82, 28


@pytest.mark.parametrize("inj", [1, 3])
def test_injected_question_gradient_hand_off_by_event(pkg, inj):
    """The full model, question at layer inj, B = 64: dq handed to the question encoder by event (per-question sums on the
    weight-gradient stream) against the synchronous hand-off (from the aligned db partials): log-probs and loss bitwise, every
    gradient to fp32 summation order; three passes each, the registry consumed every time."""
    B = 64
    RF = pkg.functional
    img = torch.from_numpy(formula.hash_uniform((B, 3, 128, 128), 341, 0.0, 1.0)).cuda()
    qst = torch.from_numpy(formula.hash_ints((B, 20), 342, 1, formula.QDICT + 1)).cuda()
    lab = torch.from_numpy(formula.hash_ints((B,), 343, 0, formula.ADICT)).cuda()

    def run(async_):
        old = RF.SCHED["dq_async"]
        RF.SCHED["dq_async"] = async_
        try:
            torch.manual_seed(11)
            m = pkg.RN(Args, dict(formula.HYP["ir-fp"], question_injection_position=inj, precision="auto", dropout=0.0)).cuda()
            m.train()
            outs = []
            for _ in range(3):
                m.zero_grad(set_to_none=True)
                lp, loss = m.forward_loss(img, qst, lab)
                n0 = RF.HANDED_BY_EVENT[0]
                loss.backward()
                torch.cuda.synchronize()
                assert RF.HANDED_BY_EVENT[0] - n0 == (1 if async_ else 0)
                assert not RF._GRAD_EVENTS
                outs.append((lp.detach().clone(), float(loss.detach()), {n_: p_.grad.clone() for n_, p_ in m.named_parameters()}))
            return outs
        finally:
            RF.SCHED["dq_async"] = old

    a, s = run(1), run(0)
    for (lp_a, loss_a, g_a), (lp_s, loss_s, g_s) in zip(a, s):
        assert torch.equal(lp_a, lp_s) and loss_a == loss_s
        for n_ in g_s:
            assert l2rel(g_a[n_].cpu().numpy(), g_s[n_].cpu().numpy()) <= 2e-5, n_
    assert float(a[0][2]["text.wembedding.weight"].abs().sum()) > 0


@pytest.mark.parametrize("inj", [1, 3])
def test_injected_eval_is_independent_of_batch_position(pkg, inj):
    """eval() runs the two-pass arithmetic (hi + lo on every layer): a question's log-probs do not depend on where it sits in the
    batch -- the reversed batch gives the reversed log-probs bitwise (whole tiles per question)."""
    B, n = 6, 64
    hyp = dict(formula.HYP["ir-fp"], question_injection_position=inj)
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], hyp)
    sd = formula.formula_rl_state(hyp, 77)
    rl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    rl = rl.cuda().eval()
    assert rl.resolved_precision(B, n, 26) == "f16s"
    x = torch.from_numpy(formula.hash_uniform((B, n, 26), 78, -1.0, 1.0)).cuda()
    q = torch.from_numpy(formula.hash_uniform((B, 128), 79, -1.0, 1.0)).cuda()
    with torch.no_grad():
        a = rl(x, q)
        b = rl(x.flip(0).contiguous(), q.flip(0).contiguous())
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    # (the tile-dithered training arithmetic moves a question's log-probs by ~1e-4 with its tile; fp32 order noise is far below 1e-6)
    assert gold.rel_err(b.flip(0).cpu().numpy(), a.cpu().numpy()) <= 1e-6


@pytest.mark.parametrize("inj", [1, 3])
def test_injected_graph_trainer_matches_eager_and_learns(inj):
    import relationnetworks_clevr_amd as pkg
    import relationnetworks_clevr_amd.train as T
    from relationnetworks_clevr_amd import dp

    def run(use_graph, steps):
        torch.manual_seed(0)
        m = pkg.RN(Args, dict(formula.HYP["ir-fp"], question_injection_position=inj, dropout=0.0)).cuda()
        assert m.rl.resolved_precision(16, 64, 26) == "f16s"
        opt = torch.optim.Adam(m.parameters(), lr=3e-4, weight_decay=1e-4)
        tr = dp.DataParallelTrainer(m, opt, clip_norm=50.0, use_graph=use_graph)
        img, q, y = T.load_tensor_data(next(iter(T.SyntheticClevr(16, 16, seed=3))), "cuda")
        return [float(tr.step(img, q, y).detach()) for _ in range(steps)]

    eager, graph = run(False, 6), run(True, 40)
    assert eager == graph[:6], (eager, graph[:6])
    assert np.isfinite(graph[-1]) and graph[-1] < 0.5 * graph[0], (graph[0], graph[-1])
