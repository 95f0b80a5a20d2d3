"""tests/normpool_ref.py (the float64 references tests/test_gpu_norm_pool_edges.py holds csrc/elementwise.hip to) is itself checked here, without
a GPU: against torch float64 autograd of the modules the network composes (BatchNorm2d -> ReLU, max_pool2d(3, 2, 1), ZeroPad2d((0,1,0,1)) ->
BatchNorm2d -> ReLU -> AvgPool2d(2), torch.optim.AdamW on a double parameter) on the planted inputs of the GPU tests, ties and exact-zero gates
included, to 1e-12 relative; and the planted inputs are held to the conditions that keep the GPU tests from being vacuous.

Two notes on the 1e-12.  (1) It is relative to the TERMS of a value (S_abs / T of the reference), not to the value: B x + C of an offset channel
cancels by design.  (2) bn_finalize takes the channel SUMS, and  var = sq / count - mu^2  from float64 sums is conditioned by kappa = 1 + mu^2 / var
(9e4 on the |mean| / std = 300 channels): two correctly rounded sums (colsums uses math.fsum) still give a variance correct only to a few
kappa 2^-53, whatever the formula is evaluated in.  Everything that hangs on such a channel's rstd is therefore held to
max(1e-12, 8 kappa 2^-53) = 8e-11 at kappa = 9e4, and to 1e-12 on the channels with |mean| / std <= 30.  The backward references are fed torch's two-pass statistics, so they are held to the plain 1e-12.

The gate is checked where it can be checked exactly: on the explicit affine relu(x * sc + sh) with the float32 (sc, sh) the kernels are handed,
whose float64 autograd has the same exact sign.  Against the BatchNorm2d module the references take the module's own mask (mask=...), because the
module forms z from float64 statistics and its near-zero signs are not those of a float32 affine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normpool_ref as nr

T64 = torch.float64
RTOL = 1e-12
POOL_SHAPES = [(1, 1, 1, 4), (1, 1, 2, 4), (1, 2, 1, 8), (2, 3, 3, 20), (3, 5, 4, 8), (2, 16, 16, 20)]
TRANS_SHAPES = [(1, 1, 1, 4), (2, 1, 6, 8), (2, 6, 1, 8), (2, 7, 9, 48), (2, 8, 10, 48)]


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


def within(got, want, tol, what):
    got, want, tol = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.broadcast_to(tol, np.shape(want))
    assert got.shape == want.shape, what
    bad = ~(np.abs(got - want) <= tol)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[0].tolist(), got[bad][0], want[bad][0], tol[bad][0])


def kappa_rtol(mean, var):
    return np.maximum(RTOL, 8 * (1.0 + mean * mean / (var + 1e-5)) * 2.0 ** -53)


def torch_bn(case, training):
    bn = torch.nn.BatchNorm2d(case["x"].shape[1]).to(T64)
    with torch.no_grad():
        bn.weight.copy_(t64(case["gamma"])); bn.bias.copy_(t64(case["beta"]))
        bn.running_mean.copy_(t64(case["rm"])); bn.running_var.copy_(t64(case["rv"]))
    return bn.train(bool(training))


# ----------------------------------------------------------------------------------
# BatchNorm -> ReLU
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("M,C", nr.BN_SHAPES)
def test_bn_references_are_torch_batchnorm(M, C, training):
    case = nr.bn_case(M, C)
    x = f = case["x"]
    s, q, sa, qa = nr.colsums(x)
    assert np.all(sa >= np.abs(s)) and np.all(np.abs(qa - q) <= 1e-13 * q)
    sc, sh, mean, rstd, rm2, rv2 = nr.bn_finalize(s, q, M, case["gamma"], case["beta"], case["rm"], case["rv"], training)
    if M == 1 and training:
        # nn.BatchNorm2d refuses one value per channel in training mode; the formula's own limit: var = 0, and the biased value is kept
        within(rstd, np.full(C, 1e-5 ** -0.5), 1e-12 * 1e-5 ** -0.5, "rstd at count 1")
        within(rv2, 0.9 * case["rv"].astype(np.float64), 1e-15, "running_var at count 1")
        within(mean, x[0].astype(np.float64), 0, "mean at count 1")
        return
    bn = torch_bn(case, training)
    xt = t64(x).reshape(M, C, 1, 1).requires_grad_(True)
    z = F.relu(bn(xt))
    gz = nr.filler.uniform(f"np.gz.{M}x{C}", (M, C), -1.0, 1.0)
    (z * t64(gz).reshape(M, C, 1, 1)).sum().backward()
    x64 = x.astype(np.float64)
    if training:
        mu_t, var_t = x64.mean(0), x64.var(0)                                      # two-pass
    else:
        mu_t, var_t = case["rm"].astype(np.float64), case["rv"].astype(np.float64)
    rs_t = 1.0 / np.sqrt(var_t + 1e-5)
    rt = kappa_rtol(mu_t, var_t) if training else RTOL
    within(mean, mu_t, RTOL * np.abs(mu_t) + 1e-300, "mean")
    within(rstd, rs_t, rt * rs_t, "rstd")
    within(sc, case["gamma"] * rs_t, rt * np.abs(case["gamma"] * rs_t), "scale")
    within(sh, case["beta"] - mu_t * case["gamma"] * rs_t, rt * (np.abs(case["beta"]) + np.abs(mu_t * case["gamma"] * rs_t)), "shift")
    within(rm2, bn.running_mean.numpy(), RTOL * (np.abs(case["rm"]) + np.abs(mu_t)), "running_mean")
    within(rv2, bn.running_var.numpy(), rt * (np.abs(case["rv"]) + var_t * (M / max(M - 1, 1))) + RTOL * np.abs(case["rv"]), "running_var")
    ch = case["special"]["const_x"]
    if ch and training:
        assert np.all(rstd[ch] == 1.0 / np.sqrt(1e-5)) and np.all(mean[ch] == 0.75)
    # backward: the module's mask, the module's statistics
    mask = z.detach().numpy().reshape(M, C) > 0
    dzm, s0, s1, a0, a1 = nr.bn_bwd_sums(gz, x, None, None, mask=mask)
    assert np.array_equal(dzm, np.where(mask, gz, 0).astype(np.float32))
    dx, dgamma, dbeta, T = nr.bn_bwd_apply(dzm, x, s0, s1, float(M), case["gamma"], mu_t, rs_t, training)
    within(dx, xt.grad.numpy().reshape(M, C), RTOL * T, "dx")
    within(dbeta, bn.bias.grad.numpy(), RTOL * a0, "dbeta")
    within(dgamma, bn.weight.grad.numpy(), RTOL * rs_t * (a1 + np.abs(mu_t) * a0), "dgamma")
    old = nr.filler.uniform(f"np.old.{M}x{C}", (M, C), -1.0, 1.0)
    dx2, _, _, T2 = nr.bn_bwd_apply(dzm, x, s0, s1, float(M), case["gamma"], mu_t, rs_t, training, old=old)
    within(dx2 - old, dx, 1e-15 * T2, "accumulate")
    assert np.array_equal(T2, T + np.abs(old))
    if C >= 8 and training:
        ch = case["special"]["g0neg"]
        assert not dx[:, ch].any() and not dgamma[ch].any() and not dbeta[ch].any()          # gamma = 0, gate closed: exact zeros


@pytest.mark.parametrize("M,C", nr.BN_SHAPES)
def test_gate_and_masked_sums_are_autograd_of_the_affine(M, C):
    """relu(x * sc + sh) with the float32 (sc, sh) a backward kernel is handed: the products are exact in float64, so torch's float64 relu backward
    has the exact sign - zero gradient at exactly 0 included - and the reference's masked dz must equal it element for element"""
    case = nr.bn_case(M, C)
    pl = nr.bn_planted(case)
    x, gz = case["x"], nr.filler.uniform(f"np.gz.{M}x{C}", (M, C), -1.0, 1.0)
    pre = (t64(x) * t64(pl["sc"]) + t64(pl["sh"])).requires_grad_(True)
    (F.relu(pre) * t64(gz)).sum().backward()
    dzm, s0, s1, a0, a1 = nr.bn_bwd_sums(gz, x, pl["sc"], pl["sh"])
    assert np.array_equal(dzm.astype(np.float64), pre.grad.numpy())
    assert np.array_equal(nr.gate(x, pl["sc"], pl["sh"]), pre.detach().numpy() > 0)
    within(s0, pre.grad.numpy().sum(0), RTOL * a0, "sum dz")
    within(s1, (pre.grad.numpy() * x).sum(0), RTOL * a1, "sum dz x")
    assert np.all(a0 >= np.abs(s0)) and np.all(a1 >= np.abs(s1))


def test_deferred_reference_is_the_per_layer_backward():
    """bn_bwd_defer over a three-layer block (running sums from zero, last layer first, each slice applied once) gives the block gradient that the
    per-layer  G[:, :cin] += B x + C  of bn_bwd_apply (A = 0 part) gives on every channel that has been applied"""
    M, C0, GR, layers = 35, 48, 48, 3
    ctot = C0 + layers * GR
    x = nr.bn_case(M, ctot, "np.defer")["x"]
    G0 = nr.filler.uniform("np.defer.G", (M, ctot), -1.0, 1.0)
    G, want = G0.astype(np.float64), G0.astype(np.float64)
    b, c = np.zeros(ctot), np.zeros(ctot)
    for i in reversed(range(layers)):
        cin = C0 + i * GR
        case = nr.bn_case(M, cin, f"np.defer.l{i}")
        pl = nr.bn_planted(dict(case, x=x[:, :cin]))
        s0 = nr.filler.uniform(f"np.defer.s0.{i}", (cin,), -4.0, 4.0, np.float64)
        s1 = nr.filler.uniform(f"np.defer.s1.{i}", (cin,), -4.0, 4.0, np.float64)
        _, B, Cc, dg, db = nr.bn_bwd_coeffs(s0, s1, float(M), pl["gamma"], pl["mean"], pl["rstd"], 1)
        want[:, :cin] += B * x[:, :cin] + Cc
        c0, n = (cin - GR, GR) if i > 0 else (0, cin)
        G, dg2, db2, b2, c2, T = nr.bn_bwd_defer(G, x[:, :cin], s0, s1, float(M), pl["gamma"], pl["mean"], pl["rstd"], b, c, c0, n, 1)
        assert np.array_equal(dg, dg2) and np.array_equal(db, db2) and not T[:, :c0].any() and not T[:, c0 + n:].any()
        b, c = np.concatenate([b2, np.zeros(ctot - cin)]), np.concatenate([c2, np.zeros(ctot - cin)])
    scale = np.abs(want).max(0) + np.abs(G0).max(0) + 1.0
    within(G[:, :C0 + (layers - 1) * GR], want[:, :C0 + (layers - 1) * GR], 1e-9 * scale[:C0 + (layers - 1) * GR], "deferred block gradient")
    assert np.array_equal(G[:, C0 + (layers - 1) * GR:], G0[:, C0 + (layers - 1) * GR:].astype(np.float64))


# ----------------------------------------------------------------------------------
# max-pool
# ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_maxpool_reference_is_torch_and_first_maximum(B, H, W, C):
    x = nr.pool_input(B, H, W, C)
    assert x.min() == 0 and np.all(x * 4 == np.round(x * 4)) and (0.3 < (x == 0).mean() < 0.7 or x.size < 64)
    if H * W >= 9:
        assert nr.tie_fraction(x) >= 0.20, nr.tie_fraction(x)
    y, arg = nr.maxpool3s2(x)
    xt = t64(x).permute(0, 3, 1, 2).requires_grad_(True)
    yt, idx = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    assert np.array_equal(y.astype(np.float64), yt.detach().permute(0, 2, 3, 1).numpy())
    # the tap code against torch's flat input index: the same element, so torch's tie rule on this build IS the first maximum
    Ho, Wo = y.shape[1:3]
    oy, ox = np.arange(Ho)[None, :, None, None], np.arange(Wo)[None, None, :, None]
    flat = (2 * oy - 1 + arg // 3) * W + (2 * ox - 1 + arg % 3)
    assert np.array_equal(flat, idx.permute(0, 2, 3, 1).numpy())
    gy = nr.filler.uniform(f"np.mp.g.{B}x{H}x{W}x{C}", y.shape, -1.0, 1.0)
    (yt * t64(gy).permute(0, 3, 1, 2)).sum().backward()
    dx, sa = nr.maxpool3s2_bwd(gy, arg, H, W)
    within(dx, xt.grad.permute(0, 2, 3, 1).numpy(), RTOL * sa, "maxpool dx")
    assert np.all(sa >= np.abs(dx))


# ----------------------------------------------------------------------------------
# transition front end
# ----------------------------------------------------------------------------------
def trans_case(B, H, W, C):
    case = nr.bn_case(B * H * W, C, "np.tp")
    return case, nr.bn_planted(case, count=B * (H + 1) * (W + 1))


@pytest.mark.parametrize("B,H,W,C", TRANS_SHAPES)
def test_padavgpool2_is_autograd_of_the_affine(B, H, W, C):
    """forward and the gated sums on the explicit float32 affine (exact signs, see the module docstring)"""
    case, pl = trans_case(B, H, W, C)
    x = case["x"].reshape(B, H, W, C)
    xp = F.pad(t64(x).permute(0, 3, 1, 2), (0, 1, 0, 1))
    pre = (xp * t64(pl["sc"]).view(1, C, 1, 1) + t64(pl["sh"]).view(1, C, 1, 1)).requires_grad_(True)
    p = F.avg_pool2d(F.relu(pre), 2)
    assert tuple(p.shape[2:]) == ((H + 1) // 2, (W + 1) // 2)
    gp = nr.filler.uniform(f"np.tp.g.{B}x{H}x{W}x{C}", (B, p.shape[2], p.shape[3], C), -1.0, 1.0)
    (p * t64(gp).permute(0, 3, 1, 2)).sum().backward()
    want_p, sabs = nr.padavgpool2(x, pl["sc"], pl["sh"])
    within(want_p, p.detach().permute(0, 2, 3, 1).numpy(), RTOL * sabs, "pooled")
    r = nr.padavgpool2_bwd(gp, x, pl["sc"], pl["sh"], pl["gamma"], pl["mean"], pl["rstd"], 1)
    dz = pre.grad.permute(0, 2, 3, 1).numpy()
    assert np.array_equal(r["dz"].astype(np.float64), dz)
    within(r["s0"], dz.sum((0, 1, 2)), RTOL * r["S0abs"], "sum dz (padded)")
    within(r["s1"], (dz * xp.permute(0, 2, 3, 1).numpy()).sum((0, 1, 2)), RTOL * r["S1abs"], "sum dz x (padded)")
    assert r["count"] == B * (H + 1) * (W + 1)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("B,H,W,C", TRANS_SHAPES)
def test_padavgpool2_backward_is_the_torch_module_chain(B, H, W, C, training):
    case, _ = trans_case(B, H, W, C)
    x = case["x"].reshape(B, H, W, C)
    bn = torch_bn(case, training)
    xt = t64(x).permute(0, 3, 1, 2).requires_grad_(True)
    z = F.relu(bn(F.pad(xt, (0, 1, 0, 1))))
    p = F.avg_pool2d(z, 2)
    gp = nr.filler.uniform(f"np.tp.g.{B}x{H}x{W}x{C}", (B, p.shape[2], p.shape[3], C), -1.0, 1.0)
    (p * t64(gp).permute(0, 3, 1, 2)).sum().backward()
    xp = F.pad(xt.detach(), (0, 1, 0, 1)).permute(0, 2, 3, 1).numpy().reshape(-1, C)
    if training:
        mu, var = xp.mean(0), xp.var(0)
    else:
        mu, var = case["rm"].astype(np.float64), case["rv"].astype(np.float64)
    rs = 1.0 / np.sqrt(var + 1e-5)
    mask = z.detach().permute(0, 2, 3, 1).numpy() > 0
    r = nr.padavgpool2_bwd(gp, x, None, None, case["gamma"], mu, rs, training, mask=mask)
    within(r["dx"], xt.grad.permute(0, 2, 3, 1).numpy(), RTOL * r["T"], "dx")
    within(r["dbeta"], bn.bias.grad.numpy(), RTOL * r["S0abs"], "dbeta")
    within(r["dgamma"], bn.weight.grad.numpy(), RTOL * rs * (r["S1abs"] + np.abs(mu) * r["S0abs"]), "dgamma")
    # the sensitivities are the derivatives of dx in the sums: a finite step in each
    if training:
        e0, e1 = 1e-3 * r["S0abs"] + 1e-6, 1e-3 * r["S1abs"] + 1e-6
        for ds0, ds1, d in ((e0, 0 * e1, r["d0"] * e0), (0 * e0, e1, r["d1"] * e1)):
            dzm = r["dz"].reshape(-1, C)
            moved = nr.bn_bwd_apply(dzm, xp, r["s0"] + ds0, r["s1"] + ds1, r["count"], case["gamma"], mu, rs, 1)[0]
            base = nr.bn_bwd_apply(dzm, xp, r["s0"], r["s1"], r["count"], case["gamma"], mu, rs, 1)[0]
            real = lambda a: a.reshape(B, H + 1, W + 1, C)[:, :H, :W]
            within(np.abs(real(moved - base)), d, 1e-6 * d + 1e-9 * r["T"], "sensitivity")


# ----------------------------------------------------------------------------------
# AdamW
# ----------------------------------------------------------------------------------
ADAMW_HP = dict(lr=float(np.float32(1e-2)), b1=float(np.float32(0.9)), b2=float(np.float32(0.999)), eps=float(np.float32(1e-8)))


@pytest.mark.parametrize("gscale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("wd", [0.0, float(np.float32(0.1))])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1027])
def test_adamw_reference_is_torch_adamw(n, wd, gscale):
    inp = nr.adamw_inputs(n)
    hp = ADAMW_HP
    p = torch.nn.Parameter(t64(inp["p"]))
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
    cur = dict(p=inp["p"].astype(np.float64), m=np.zeros(n), v=np.zeros(n))
    for step, g in ((1, inp["g"]), (2, inp["g2"])):                               # the moments are carried
        p.grad = t64(g) * gscale
        opt.step()
        r = nr.adamw(cur["p"], g, cur["m"], cur["v"], step, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, gscale)
        st = opt.state[p]
        within(r["m"], st["exp_avg"].numpy(), RTOL * r["Tm"], "m")
        within(r["v"], st["exp_avg_sq"].numpy(), RTOL * r["Tv"], "v")
        within(r["p"], p.detach().numpy(), RTOL * (np.abs(cur["p"]) + np.abs(r["update"])), "p")
        if step == 1:
            assert np.all(r["v"][inp["zero"]] == 0) and np.all(r["denom"][inp["zero"]] == hp["eps"]) and not r["update"][inp["zero"]].any()
        cur = r
    # step 1000 on planted moments
    p = torch.nn.Parameter(t64(inp["p"]))
    opt = torch.optim.AdamW([p], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=wd)
    opt.state[p] = dict(step=torch.tensor(999.0), exp_avg=t64(inp["m0"]), exp_avg_sq=t64(inp["v0"]))
    p.grad = t64(inp["g"]) * gscale
    opt.step()
    r = nr.adamw(inp["p"], inp["g"], inp["m0"], inp["v0"], 1000, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, gscale)
    assert float(opt.state[p]["step"]) == 1000.0
    within(r["p"], p.detach().numpy(), RTOL * (np.abs(inp["p"]) + np.abs(r["update"])), "p at step 1000")
    within(r["m"], opt.state[p]["exp_avg"].numpy(), RTOL * r["Tm"], "m at step 1000")
    within(r["v"], opt.state[p]["exp_avg_sq"].numpy(), RTOL * r["Tv"], "v at step 1000")
    if n >= 1027:                                                                  # the update dominates the value
        assert np.median(np.abs(r["update"][~inp["zero"]])) > 3 * np.abs(inp["p"]).max()


# ----------------------------------------------------------------------------------
# the planted inputs: conditions that keep the GPU tests from being vacuous
# ----------------------------------------------------------------------------------
def teeth_channels(case, M):
    """channels on which dropping ANY single row moves the float64 sums by more than the GPU tolerance 2^-16 S_abs: the offset channels, whose
    terms share a sign and a size, so each is about S_abs / M > 2^-16 S_abs for M < 65 536.  |mean| / std >= 30 at every M; |mean| / std = 3 as
    well up to M = 570 (its smallest term is ~0.4 of the mean one, too little at M = 24 593); M = 1: every channel with a non-zero value."""
    ratio, M_ = case["ratio"], M
    if M_ == 1:
        return np.flatnonzero(case["x"][0] != 0)
    return np.flatnonzero(ratio >= (3.0 if M_ <= 570 else 30.0))


@pytest.mark.parametrize("M,C", nr.BN_SHAPES)
def test_planted_bn_inputs_meet_their_conditions(M, C):
    case = nr.bn_case(M, C)
    pl = nr.bn_planted(case)
    x, sp = case["x"], case["special"]
    assert x.dtype == np.float32 and pl["sc"].dtype == np.float32 and pl["sh"].dtype == np.float32
    assert nr.gate_zero_fraction(x, pl["sc"], pl["sh"]) >= 0.01                                  # x * sc + sh exactly 0
    assert (pl["sc"] < 0).sum() >= 1
    if C >= 8:
        assert all(len(sp[k]) >= 1 for k in ("zero_x", "const_x", "g0neg", "g0pos", "tiny"))
        assert np.all(pl["sc"][sp["g0pos"]] == 0) and np.all(pl["sh"][sp["g0pos"]] > 0)
        assert np.all(pl["sc"][sp["g0neg"]] == 0) and np.all(pl["sh"][sp["g0neg"]] < 0)
        assert np.all(x[:, sp["const_x"]] == 0.75) and not x[:, sp["zero_x"]].any()
        assert np.all(case["gamma"][sp["tiny"]] == np.float32(1e-6))
    if C >= 16:
        for k, tie, s_, t_ in (("tie_pos", 0.5, 2.0, -1.0), ("tie_neg", 0.25, -4.0, 1.0)):
            ch = sp[k]
            assert len(ch) and np.all(pl["sc"][ch] == s_) and np.all(pl["sh"][ch] == t_) and (x[:, ch] == tie).mean() > 0.3
    if M >= 35:                                                                                  # every |mean| / std of the recipe is there
        x64 = x.astype(np.float64)
        got = np.abs(x64.mean(0)) / (x64.std(0) + 1e-30)
        for ratio in (3.0, 30.0, 300.0):
            ch = np.flatnonzero(case["ratio"] == ratio)
            assert len(ch) and np.all(np.abs(got[ch] / ratio - 1) < 0.35), (ratio, got[ch])
    # teeth of the statistics cases
    s, q, sa, qa = nr.colsums(x)
    ch = teeth_channels(case, M)
    assert len(ch) >= 1
    x64 = x.astype(np.float64)
    assert np.all(np.abs(x64[:, ch]).min(0) > 2.0 ** -16 * sa[ch]), "dropping a row from sum x"
    assert np.all((x64[:, ch] ** 2).min(0) > 2.0 ** -16 * qa[ch]), "dropping a row from sum x^2"


@pytest.mark.parametrize("B,H,W,C", TRANS_SHAPES)
def test_planted_transition_inputs_meet_their_conditions(B, H, W, C):
    case, pl = trans_case(B, H, W, C)
    assert nr.gate_zero_fraction(case["x"], pl["sc"], pl["sh"]) >= 0.01
    assert (pl["sc"] < 0).sum() >= 1
    # a padded pixel's value is relu(shift): the recipe opens some channels' padding and closes others' decisively
    if C >= 8:
        lim = 1.0 if C >= 48 else 0.25
        assert (pl["sh"] > lim).sum() >= 1 and (pl["sh"] < -lim).sum() >= 1
