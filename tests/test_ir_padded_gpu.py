"""GPU: ir-fp (the question injected at g layer 2) on the padded j axis of the f16s chain (n % 32 != 0): the forward kernel's new
variants against the float64 emulation of their arithmetic (tiles that straddle two questions read each wave's own question row),
parity with the reference's fixtures (tests/golden/make_golden_ir_padded.py), both sources of the injected layer's question sums,
the question gradient handed over by event, the batch-independent eval arithmetic, and the graph-replayed trainer."""
import numpy as np
import pytest
import torch

import gold
from oracle import formula
from test_gpu_kernels import F16S_V, check_against_f16s_emulation, dev, dither_images, f16s_images, rr_mask_decode, unblock, unblock_h
from test_gpu_parity import F16S_GUARD, l2rel, report

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


def inj_padded_emulation(x, Vq, Ws, bs, n, njp, inj=2):
    """float64 emulation of the f16s chain with the question at layer inj on the PADDED pair space (row (b, i, j), j < njp; the rows
    j >= n multiply the zero object row and are invalid).  -> (pre-activations, valid rows, the exact chain's last layer)."""
    B, _, k = x.shape
    G, L = 256, len(Ws)
    f16r = lambda a: np.asarray(a, np.float32).astype(np.float16).astype(np.float32)
    M = B * n * njp
    r = np.arange(M)
    b_of, i_of, j_of = r // (n * njp), (r // njp) % n, r % njp
    valid = j_of < n
    xj = x[b_of, np.minimum(j_of, n - 1)] * valid[:, None]
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
    return zs, valid, exact


@pytest.mark.parametrize("B,n", [(200, 12), (8, 36), (2, 196)])
def test_g_chain_fwd_rr_f16s_alg0_ir_padded(H, B, n):
    """rn_g_chain_fwd_rr_f16s_alg0 with inject_layer 2 on the padded j axis.  n = 12 (384 rows per question): every other tile holds
    two questions (waves 0..3 / 4..7), 300 tiles -- workgroups carry both rows of the next tile; n = 36: padded, no tile straddles;
    n = 196: tile 171 straddles.
    16-bit copies, masks and the two partial pair-sum rows per tile against the emulation, padded rows with cleared masks, the
    per-question sums of rn_pair_sum_tiles against the exact chain; the e4m3, gate and inference variants against that run."""
    L, G, k, Q, inj = 4, 256, 26, 128, 2
    njp = (n + 31) // 32 * 32
    Mp, kt = B * n * njp, 2 * k
    assert Mp % 256 == 0
    x = formula.hash_uniform((B, n, k), 600 + n, -1, 1).astype(np.float32)
    q = formula.hash_uniform((B, Q), 610 + n, -1, 1).astype(np.float32)
    Ws = [formula.hash_uniform((G, kt if l == 0 else G + (Q if l == inj else 0)), 620 + l, -0.15, 0.15).astype(np.float32) for l in range(L)]
    bs = [formula.hash_uniform((G,), 630 + l, -0.3, 0.3).astype(np.float32) for l in range(L)]
    Vq = (q.astype(np.float64) @ Ws[inj][:, G:].T.astype(np.float64) + bs[inj]).astype(np.float32)
    wd = [dev(w) for w in Ws]
    w0T = torch.empty(kt, G, device="cuda")
    his, lo0, jobs = f16s_images(H, wd, kt, k)
    jobs = [j if j[0] is not wd[inj] else (wd[inj], G + Q, 1, G, G, his[inj], j[6]) for j in jobs]   # (the H columns of W_inj)
    H.pack_matrix_frag_many(jobs + [(wd[0], kt, 1, G, kt, w0T, 2)])
    Xp = torch.zeros(B * n + 1, 64, dtype=torch.float16, device="cuda"); Vc = torch.empty(B * n, G, device="cuda")
    H.pair_tables(dev(x), None, w0T, dev(bs[0]), Xp, Vc, B, n, k, 0, G)
    bd, Vqd = [dev(b) for b in bs], dev(Vq)

    def run(dtype, gate=False, store=True):
        Hs = masks = None
        if store and dtype == torch.bfloat16:
            Hs = [torch.full((Mp, G), float("nan"), dtype=torch.bfloat16, device="cuda") for _ in range(3)] + [None]
        elif store:
            Hs = [torch.full((Mp, G), 0x7f, dtype=torch.uint8, device="cuda").view(dtype) for _ in range(3)] + [None]
        if store:
            masks = list(torch.full((L, H.g_chain_rr_mask_bytes(Mp)), 0xff, dtype=torch.uint8, device="cuda"))
        part = torch.full((Mp // 256 * 2, G), float("nan"), dtype=torch.float32, device="cuda")
        H.g_chain_fwd_rr_f16s_alg0(Xp, Vc, n, his, lo0, bd, Hs, masks, part, Mp, G, Vq=Vqd, inject=inj, njp=njp, gate=gate)
        torch.cuda.synchronize()
        return Hs, masks, part

    Hs16, m16, p16 = run(torch.bfloat16)
    Hs16 = unblock_h(Hs16)
    zs, valid, exact = inj_padded_emulation(x, Vq, Ws, bs, n, njp, inj)
    check_against_f16s_emulation(zs, valid, exact, Hs16, m16, p16, Mp, n_parts_per_tile=2, grp_tol=1e-3)
    for l in range(L):
        assert not torch.from_numpy(rr_mask_decode(m16[l], Mp, l)).view(B * n, njp, G)[:, n:].any(), l   # (padded rows: cleared)
    # the two partial rows of a straddling tile: each is the sum over ITS question's rows of the tile
    last = np.maximum(zs[-1], 0) * valid[:, None]
    rq = np.arange(Mp) // (n * njp)
    pp = p16.cpu().numpy().reshape(Mp // 256, 2, G)
    for t in sorted({int(t) for t in np.nonzero(rq[::256] != rq[255::256])[0]})[:4]:
        rows = slice(256 * t, 256 * t + 256)
        first = rq[rows] == rq[256 * t]
        assert 0 < first.sum() < 256
        assert l2rel(pp[t, 0], last[rows][first].sum(0)) <= 1e-3 and l2rel(pp[t, 1], last[rows][~first].sum(0)) <= 1e-3, t
    xg = torch.full((B, G), float("nan"), device="cuda")
    H.pair_sum_tiles(p16, xg, Mp, n * njp, G)
    torch.cuda.synchronize()
    # (against the emulated arithmetic: a 12-object question spans 1.5 tiles, too few for the dithered roundings to average out)
    assert l2rel(xg.cpu().numpy(), last.reshape(B, n * njp, G).sum(1)) <= 1e-3
    # e4m3 copies, then the gate in the sign bits of H_2: masks and pair sums bitwise those of the 16-bit run
    Hs8, m8, p8 = run(torch.float8_e4m3fn)
    Hg, mg, pg = run(torch.float8_e4m3fn, gate=True)
    assert torch.equal(p8, p16) and torch.equal(pg, p16)
    for l in range(L):
        assert torch.equal(m8[l], m16[l]) and torch.equal(mg[l], m16[l]), l
    for l in range(2):
        assert torch.equal(Hg[l].view(torch.uint8), Hs8[l].view(torch.uint8)), l
    want = H.relu_gate_image(m8[3], Hs8[2].clone(), Mp)
    torch.cuda.synchronize()
    assert torch.equal(Hg[2].view(torch.uint8), want.view(torch.uint8))
    assert not (unblock(Hg[2]).view(torch.uint8) >> 7).view(B * n, njp, G)[:, n:].any()
    # inference: one pass (bitwise the training run's pair sums), and two passes (hi + lo on every layer) against the exact chain
    _, _, pi = run(None, store=False)
    assert torch.equal(pi, p16)
    his2 = [torch.empty(1, 65536, dtype=torch.float16, device="cuda") for _ in range(L)]
    los2 = [torch.empty(65536, dtype=torch.float16, device="cuda") for _ in range(L)]
    j2 = [(wd[0], kt, 1, G, k, his2[0], 4 | 1), (wd[0], kt, 1, G, k, los2[0], 8 | 1)]
    j2 += [(wd[l], Ws[l].shape[1], 1, G, G, his2[l], 4) for l in range(1, L)] + [(wd[l], Ws[l].shape[1], 1, G, G, los2[l], 8) for l in range(1, L)]
    H.pack_matrix_frag_many(j2)
    p2 = torch.full((Mp // 256 * 2, G), float("nan"), dtype=torch.float32, device="cuda")
    H.g_chain_fwd_rr_f16s_alg0(Xp, Vc, n, his2, los2, bd, None, None, p2, Mp, G, Vq=Vqd, inject=inj, njp=njp)
    torch.cuda.synchronize()
    got2 = p2.cpu().numpy().reshape(Mp // 256, 2, G).sum(1)
    assert l2rel(got2, (exact * valid[:, None]).reshape(Mp // 256, 256, G).sum(1)) <= 1e-3


def run_rl(pkg, g, precision, x=None, q=None):
    meta = g["meta"]
    hyp, sd, x0, q0, lab = gold.rl_case(meta)
    x = x0 if x is None else x
    q = q0 if q is None else q
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], dict(hyp, precision=precision))
    rl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    rl = rl.cuda().eval()
    if meta.get("strided"):
        xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 2, 1))).cuda().permute(0, 2, 1)
    else:
        xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    xt.requires_grad_(True)
    qt = torch.from_numpy(np.ascontiguousarray(q)).cuda().requires_grad_(True)
    lp = rl(xt, qt)
    loss = torch.nn.functional.nll_loss(lp, torch.from_numpy(lab).cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {n_: p_.grad.detach().cpu().numpy() for n_, p_ in rl.named_parameters()}
    return lp.detach().cpu().numpy(), float(loss.detach()), xt.grad.cpu().numpy(), qt.grad.cpu().numpy(), grads, rl


@pytest.mark.parametrize("precision", ["auto", "f16s", "fp32"])
def test_ir_fp_stress_grid_parity(pkg, precision):
    """ir-fp on the 14 x 14 grid, B = 32 (G-ir196-b32, recorded from the reference at this size): "auto" / "f16s" run the chain on the
    padded j axis with the question row at layer 2; the bars of test_stress_config_real_dispatch."""
    g = gold.load("G-ir196-b32")
    meta = g["meta"]
    assert meta["b"] == 32 and meta["n"] == 196
    lp, loss, dx, dq, grads, rl = run_rl(pkg, g, precision)
    assert rl.resolved_precision(32, 196, 26) == ("fp32" if precision == "fp32" else "f16s")
    e_lp = gold.rel_err(lp, g["log_probs"])
    e_dq = l2rel(dq, g["dq"])
    e_dxs = l2rel(dx.reshape(-1)[g["dx_sample_idx"]], g["dx_sample"])
    e_dxn = abs(float(np.linalg.norm(dx.astype(np.float64))) - float(g["dx_norm"])) / float(g["dx_norm"])
    e_b = max(l2rel(grads[k_[5:]], g[k_]) for k_ in g if k_.startswith("grad/"))
    e_wn = max(abs(float(np.linalg.norm(grads[k_[9:]].astype(np.float64))) - float(g[k_])) / max(float(g[k_]), 1e-30)
               for k_ in g if k_.startswith("gradnorm/"))
    agree = float((lp.argmax(1) == g["log_probs"].argmax(1)).mean())
    report("G-ir196-b32", precision=precision, log_probs=e_lp, dq_l2=e_dq, dx_sample_l2=e_dxs, dx_norm=e_dxn, bias_l2=e_b, wnorm=e_wn,
           argmax_agree=agree)
    lp_tol, g_tol = {"fp32": (1e-5, 1e-3), "f16s": (F16S_GUARD, 1.2e-2), "auto": (F16S_GUARD, 1.2e-2)}[precision]
    assert np.isfinite(lp).all() and e_lp <= lp_tol
    assert e_dq <= g_tol and e_dxs <= g_tol and e_dxn <= g_tol and e_b <= g_tol and e_wn <= g_tol, (e_dq, e_dxs, e_dxn, e_b, e_wn)
    assert agree == 1.0


@pytest.mark.parametrize("precision", ["f16s", "fp32"])
def test_ir_fp_straddling_small_parity(pkg, precision):
    """G-ir196-small: B = 2, n = 196 -- tile 171 holds the end of question 0 and the start of question 1; every gradient recorded."""
    g = gold.load("G-ir196-small")
    lp, loss, dx, dq, grads, _ = run_rl(pkg, g, precision)
    e_lp, e_dx, e_dq = gold.rel_err(lp, g["log_probs"]), l2rel(dx, g["dx"]), l2rel(dq, g["dq"])
    e_w = gold.check_grads(g, grads, 3e-2 if precision == "f16s" else 1e-3, {})
    report("G-ir196-small", precision=precision, log_probs=e_lp, dx_l2=e_dx, dq_l2=e_dq, params=e_w)
    if precision == "fp32":
        assert e_lp <= 1e-5 and e_dx <= 1e-3 and e_dq <= 1e-3
    else:
        assert e_lp <= F16S_GUARD and e_dx <= 2e-2 and e_dq <= 2e-2, (e_lp, e_dx, e_dq)


@pytest.mark.parametrize("tag", ["G-ir196-b32", "G-ir196-small"])
def test_ir_padded_question_sums_from_either_source(pkg, tag, monkeypatch):
    """Rq of layer 2 from the weight-gradient launch's question-aligned db partials (rows per question = n * njp), or from
    rn_blocked_question_sums over the stored padded dZ_2 (forced by hiding the aligned split count): forward and dx bitwise, dq
    and the g-layer gradients to 1e-5, the rest bitwise."""
    g = gold.load(tag)
    real = pkg.rn_hip.wgrad_blocked_splits
    monkeypatch.setattr(pkg.rn_hip, "wgrad_blocked_splits", lambda M, rpq=0, njobs=1, aligned=False: 0 if aligned else real(M, rpq, njobs, aligned))
    lp0, _, dx0, dq0, gr0, _ = run_rl(pkg, g, "f16s")
    monkeypatch.setattr(pkg.rn_hip, "wgrad_blocked_splits", real)
    lp1, _, dx1, dq1, gr1, _ = run_rl(pkg, g, "f16s")
    assert np.array_equal(lp0, lp1) and np.array_equal(dx0, dx1)
    report(tag, precision="f16s", rq_sources_dq_l2=l2rel(dq1, dq0))
    assert l2rel(dq1, dq0) <= 1e-5
    for k in gr0:
        if k.startswith("g_layers.") and not k.startswith("g_layers.0."):
            assert l2rel(gr1[k], gr0[k]) <= 1e-5, k
        else:
            assert np.array_equal(gr0[k], gr1[k]), k


class Args:
    qdict_size, adict_size = 82, 28


@pytest.mark.parametrize("hw", [96, 224])
def test_ir_padded_question_gradient_hand_off_by_event(pkg, hw):
    """The full ir-fp model on a 6 x 6 (hw = 96: n = 36) and a 14 x 14 grid (hw = 224: n = 196, straddling tiles), B = 8: dq handed
    to the question encoder by event against the synchronous hand-off -- log-probs and loss bitwise, every gradient to fp32
    summation order; two passes each."""
    B = 8
    RF = pkg.functional
    img = torch.from_numpy(formula.hash_uniform((B, 3, hw, hw), 351, 0.0, 1.0)).cuda()
    qst = torch.from_numpy(formula.hash_ints((B, 20), 352, 1, formula.QDICT + 1)).cuda()
    lab = torch.from_numpy(formula.hash_ints((B,), 353, 0, formula.ADICT)).cuda()

    def run(async_):
        old = RF.SCHED["dq_async"]
        RF.SCHED["dq_async"] = async_
        try:
            torch.manual_seed(11)
            m = pkg.RN(Args, dict(formula.HYP["ir-fp"], precision="auto", dropout=0.0)).cuda()
            m.train()
            outs = []
            for _ in range(2):
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


@pytest.mark.parametrize("B,n", [(6, 196), (6, 36)])
def test_ir_padded_eval_is_independent_of_batch_position_and_object_order(pkg, B, n):
    """eval() runs the two-pass arithmetic: a question's log-probs do not depend on where it sits in the batch (the reversed batch
    moves the tile boundaries between questions) nor on the order of its objects -- up to fp32 summation order."""
    hyp = dict(formula.HYP["ir-fp"])
    rl = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], hyp)
    sd = formula.formula_rl_state(hyp, 87)
    rl.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    rl = rl.cuda().eval()
    assert rl.resolved_precision(B, n, 26) == "f16s"
    x = torch.from_numpy(formula.hash_uniform((B, n, 26), 88, -1.0, 1.0)).cuda()
    q = torch.from_numpy(formula.hash_uniform((B, 128), 89, -1.0, 1.0)).cuda()
    perm = torch.from_numpy(np.random.RandomState(5).permutation(n)).cuda()
    with torch.no_grad():
        a = rl(x, q)
        b = rl(x.flip(0).contiguous(), q.flip(0).contiguous())
        c = rl(x[:, perm].contiguous(), q)
        ref = pkg.RelationalLayer(hyp["rl_in_size"], formula.ADICT, hyp["lstm_hidden"], dict(hyp, precision="fp32")).cuda().eval()
        ref.load_state_dict(rl.state_dict())
        r = ref(x, q)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    e_b, e_c = gold.rel_err(b.flip(0).cpu().numpy(), a.cpu().numpy()), gold.rel_err(c.cpu().numpy(), a.cpu().numpy())
    e_r = gold.rel_err(a.cpu().numpy(), r.cpu().numpy())
    report("ir-padded-eval-%d" % n, batch_position=e_b, object_order=e_c, two_pass_vs_fp32=e_r)
    assert e_b <= 5e-5 and e_c <= 5e-5, (e_b, e_c)
    assert e_r <= 1e-3


def test_ir_padded_graph_trainer_matches_eager_and_learns():
    """The graph-replayed trainer on ir-fp at a padded shape (6 x 6 grid, hw = 96: n = 36, njp = 64) equals the eager steps."""
    import relationnetworks_clevr_amd as pkg
    import relationnetworks_clevr_amd.train as T
    from relationnetworks_clevr_amd import dp

    def run(use_graph, steps):
        torch.manual_seed(0)
        m = pkg.RN(Args, dict(formula.HYP["ir-fp"], dropout=0.0)).cuda()
        assert m.rl.resolved_precision(16, 36, 26) == "f16s"
        opt = torch.optim.Adam(m.parameters(), lr=3e-4, weight_decay=1e-4)
        tr = dp.DataParallelTrainer(m, opt, clip_norm=50.0, use_graph=use_graph)
        img, q, y = T.load_tensor_data(next(iter(T.SyntheticClevr(16, 16, hw=96, seed=3))), "cuda")
        assert img.shape[-1] == 96
        return [float(tr.step(img, q, y).detach()) for _ in range(steps)]

    eager, graph = run(False, 6), run(True, 40)
    assert eager == graph[:6], (eager, graph[:6])
    assert np.isfinite(graph[-1]) and graph[-1] < 0.5 * graph[0], (graph[0], graph[-1])
