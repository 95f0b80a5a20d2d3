"""tests/wsm_ref.py without a GPU: the references against independent formulations, and the PLANTED INPUTS of every case of
tests/test_gpu_wsm_exact.py against the conditions under which its tolerance is zero:
  (a) operands: activations and weights integers in [-4, 4], biases multiples of 1/4 with |b| <= 8 (exact in bf16 / f32);
  (b) exact accumulation: sum |x||w| + |b| < 2^22 per output, so every f32 summation order and the bias add are exact;
  (c) rounding is exercised: every bf16-output case with K >= 256 holds outputs that are no bf16 numbers and round up, that round down, exact ties
      whose even neighbour lies above and ties whose even neighbour lies below (counted, not planted);
  (d) the tile rule: the tile each case names is what launch_wsm_conv_bf16 picks, <4,2> iff ceil(M/128) * ceil(N/64) >= 512.  The launcher
      records no census entry, so this is a restatement of the code (wsm_ref.tile), recomputed here for every case;
  (e) the chain: every tensor the bf16 chain stores (t, out1, the five conv1_k outputs, the five slots) of the float64 restatement is a bf16
      number, and sum |x||w| + |b| < 2^24 at conv1, whose integer sums are then exact in f32.
These are conditions on the inputs and the reference alone, not measurements of a kernel.  Power: each packing / routing mutation of
wsm_ref.mutations changes the expected map of the planted d_7, so equality on the GPU cannot hold with the corresponding error."""
import numpy as np
import pytest
import torch

import wsm_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300)


# ---- the references against independent formulations (explicit shifted sums over the taps) -----------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 5])
def test_conv_reference(k):
    B, H, W, cin, n = 2, 3, 4, 5, 6
    x = R.filler.uniform("wr.x%d" % k, (B * H * W, cin), -2, 2, np.float64)
    w = R.filler.uniform("wr.w%d" % k, (n, cin, k, k), -1, 1, np.float64)
    b = R.filler.uniform("wr.b", (n,), -1, 1, np.float64)
    xp = np.zeros((B, H + k - 1, W + k - 1, cin))
    xp[:, k // 2:k // 2 + H, k // 2:k // 2 + W] = x.reshape(B, H, W, cin)
    want = sum(np.einsum("bhwc,nc->bhwn", xp[:, r:r + H, s:s + W], w[:, :, r, s]) for r in range(k) for s in range(k)).reshape(-1, n) + b
    got, mag = R.conv_ref(x, w, b, B, H, W)
    close(got, want)
    close(mag, R.conv_ref(np.abs(x), np.abs(w), np.abs(b), B, H, W)[0])
    close(R.conv_ref(x, w, None, B, H, W)[0], want - b)


def test_deconv_reference():
    B, h, wd, cin, c = 2, 3, 2, 5, 6
    x = R.filler.uniform("wr.dx", (B * h * wd, cin), -2, 2, np.float64)
    w = R.filler.uniform("wr.dw", (cin, c, 2, 2), -1, 1, np.float64)
    b = R.filler.uniform("wr.db", (c,), -1, 1, np.float64)
    want = np.zeros((B, 2 * h, 2 * wd, c))
    for r in range(2):
        for s in range(2):
            want[:, r::2, s::2] = np.einsum("bhwi,io->bhwo", x.reshape(B, h, wd, cin), w[:, :, r, s]) + b
    close(R.deconv_ref(x, w, b, B, h, wd)[0], want.reshape(-1, c))


@pytest.mark.parametrize("columns", [0, 1])
def test_strip_reference(columns):
    B, S, ci, n = 3, 4, 5, 6
    x = R.filler.uniform("wr.sx", (B * S * S, ci), -2, 2, np.float64)
    w = R.filler.uniform("wr.sw%d" % columns, (n, ci, S, 3) if columns else (n, ci, 3, S), -1, 1, np.float64)
    b = R.filler.uniform("wr.sb", (n,), -1, 1, np.float64)
    m = x.reshape(B, S, S, ci)
    want = np.zeros((B, S, n))
    for t in range(S):                                     # the value of row (column) t: rows (columns) t-1, t, t+1, zero outside THIS image
        for d in range(3):
            u = t + d - 1
            if 0 <= u < S:
                want[:, t] += np.einsum("bpc,ncp->bn", m[:, :, u], w[:, :, :, d]) if columns else np.einsum("bpc,ncp->bn", m[:, u], w[:, :, d, :])
    got, mag = R.strip_values(x, w, b, B, S, columns)
    close(got, want + b)
    full = R.strip_broadcast(got, columns).reshape(B, S, S, n)
    for t in range(S):
        assert np.array_equal(full[:, :, t] if columns else full[:, t], np.broadcast_to(got[:, t][:, None], (B, S, n)))


def test_layout_helpers():
    xin = R.ints("wr.px", (3, 40), -4, 4)
    x = R.place_x(xin, 80, 8, 40)
    assert x.shape == (3 * 80 + 64,) and np.isnan(x[-64:]).all() and not np.isnan(x[:-64]).any()
    rows = x[:-64].reshape(3, 80)
    assert np.array_equal(rows[:, 8:48], xin) and (rows[:, 48:72] == R.PAD).all() and (rows[:, :8] == R.BIG).all() and (rows[:, 72:] == R.BIG).all()
    assert (R.place_x(xin, 40, 0, 40)[:-64].reshape(3, 40) == xin).all()
    wt = R.ints("wr.pw", (5, 9, 40), -4, 4)
    wp = R.pack_rows(wt, 40).reshape(64, 9, 64)
    assert np.array_equal(wp[:5, :, :40], wt) and not wp[:5, :, 40:].any() and (wp[5:] == R.BIG).all()
    v = R.with_ties("wr.t", (4, 1056, 8, 8), -3.0, 3.0)
    c = R.rounding_counts(v)
    assert min(c.values()) > 1000
    out = R.nchw_to_nhwc(v, 1064)
    assert np.isnan(out[:, 1056:]).all() and np.array_equal(out[64 + 9, :1056], R.round_bf16(v[1, :, 1, 1])[0])
    assert R.rounding_counts(np.array([257.0, 259.0, 513.0, 515.0, -257.0, -259.0, 3.0])) == dict(up=1, down=1, tie_above=2, tie_below=2)


# ---- the planted inputs of every GPU case -------------------------------------------------------------------------------------------------------
def hold(c, bf16_out=True, what=""):
    assert R.operands_ok(c), what                                                         # (a)
    assert R.exact_sum(c["mag"]) < R.LIMIT, (what, R.exact_sum(c["mag"]))                 # (b)
    assert np.array_equal(c["exact"].astype(np.float32).astype(np.float64), c["exact"])
    if bf16_out and c["K"] >= 256:                                                        # (c)
        counts = R.rounding_counts(c["exact"])
        assert min(counts.values()) >= 1, (what, counts)
    wp = c["wp"]                                                                          # the packer's contract and the poison
    n = c["N"] if "c" not in c else None
    if n is not None:
        assert (wp[n:] == R.BIG).all() and wp.shape[0] == R.p64(n) and wp.shape[1] == c["K"]
        assert np.abs(wp[:n]).max() <= 4
    assert np.isnan(c["x"][-64:]).all() and not np.isnan(c["x"][:-64]).any()


@pytest.mark.parametrize("name", sorted(R.CONV_CASES))
def test_conditions_conv(name):
    B, H, W, cin, n, k, ldx, xoff, bias = R.CONV_CASES[name]
    c = R.build_conv(name)
    hold(c, True, name)
    assert R.tile(c["M"], n) == R.TILES[name]                                             # (d)
    assert ldx % 8 == 0 and xoff % 8 == 0 and ldx >= xoff + cin and (c["b"] is None) == (not bias)
    for coff, ldc in R.STORES[name]:
        assert ldc >= coff + n
    wp = c["wp"].reshape(R.p64(n), k * k, R.p32(cin))
    assert not wp[:n, :, cin:].any()                                                      # weight columns ci in [cin, pad32(cin)) of every tap are zero
    taps = ([(k // 2, k // 2 + 1)] if k > 1 and W > 1 else []) + ([(0, k - 1)] if k > 1 and min(H, W) > k // 2 else [])
    for r, s in taps:                                                                     # teeth: the right neighbour's tap / a corner tap removed
        wd = c["w"].copy()
        wd[:, :, r, s] = 0.0
        assert (R.conv_ref(c["xin"], wd, c["b"], B, H, W)[0] != c["exact"]).any()


def test_conditions_conv_axes():
    """the case table holds what it was shaped for: the K steps, the store paths, the tile threshold from both sides"""
    assert [(R.p32(cin), R.k_steps(R.p32(cin))) for cin in R.K_AXIS] == list(R.K_AXIS.values()) == [(32, 1), (64, 1), (96, 2), (160, 3), (192, 3), (224, 4), (288, 5)]
    assert {R.p32(cin) % 64 for cin in R.K_AXIS} == {32, 0}
    assert sorted(M for M in R.M_AXIS) == [1, 33, 64, 65, 105] and all(B * H * W == M for M, (B, H, W) in R.M_AXIS.items())
    assert R.N_AXIS == (1, 10, 26, 52, 64, 65, 130)
    for n in R.N_AXIS:
        assert R.STORES["k1_n%d" % n][:4] == ((0, n + 12), (4, n + 12), (2, n + 10), (3, n + 9))
    assert R.STORES["k1_n26"][4:] == ((156, 208), (182, 208))                             # the real slot offsets 3 ki and 3 ki + wi of C = 208
    assert R.CONV_CASES["k1_c40_ld40"][6] % 32 and R.CONV_CASES["k1_c208_ld208"][6] % 32  # ldx no multiple of 32: NaN sits behind the last element
    assert R.build_conv("k5_c40")["K"] == 1600
    M42, M22 = R.build_conv("t42_k1")["M"], R.build_conv("t22_k1")["M"]
    assert (M42, R.cdiv(M42, 128) * R.cdiv(450, 64), M22, R.cdiv(M22, 128) * R.cdiv(450, 64)) == (8125, 512, 8064, 504)
    assert R.tile(8125, 450) == "<4,2>" and R.tile(8064, 450) == "<2,2>" and R.tile(2 * 64 * 65, 450) == "<4,2>"
    cin, c, B, h, w = R.DECONV_TILE_CASE
    assert R.tile(B * h * w, 4 * R.p32(c)) == "<4,2>" and 4 * R.p32(c) == 512


@pytest.mark.parametrize("cc", R.DECONV_CC + (R.DECONV_TILE_CASE[:2],), ids=lambda cc: "cin%d_c%d" % cc)
def test_conditions_deconv(cc):
    cin, c = cc
    assert c % 4 or c % 32
    geoms = R.DECONV_GEOMS if cc in R.DECONV_CC else (R.DECONV_TILE_CASE[2:],)
    for B, h, w in geoms:
        d = R.build_deconv(cin, c, B, h, w)
        hold(d, True, (cc, B, h, w))
        assert d["exact"].shape == (B * 4 * h * w, c) and d["ldc"] == c + 8
        cp = R.p32(c)
        wp = d["wp"].reshape(4, cp, R.p32(cin))
        assert np.abs(wp[:, :c]).max() <= 4 and (wp[:, c:] == R.BIG).all() and not d["b"].reshape(4, cp)[:, c:].any()
        assert all(np.array_equal(d["b"].reshape(4, cp)[ph, :c], d["b"][:c]) for ph in range(4))
        if cc in R.DECONV_CC:
            assert R.tile(d["M"], d["N"]) == "<2,2>"
        ws = np.ascontiguousarray(d["w"].transpose(0, 1, 3, 2))                           # teeth: the phases (r, s) swapped
        assert (R.deconv_ref(d["xin"], ws, d["b"][:c], B, h, w)[0] != d["exact"]).any()


@pytest.mark.parametrize("columns", [0, 1])
@pytest.mark.parametrize("name", sorted(R.STRIP_CASES))
def test_conditions_strip(name, columns):
    S, cw, n, B, xoff, coff = R.STRIP_CASES[name]
    c = R.build_strip(name, columns)
    hold(c, True, (name, columns))
    assert c["K"] == 3 * S * cw and R.tile(c["M"], n) == "<2,2>" and c["ldx"] > xoff + cw and c["ldc"] > coff + n
    wp = c["wp"].reshape(R.p64(n), 3 * S, cw)
    assert not wp[:n, :, cw - 6:].any() and c["exact"].shape == (B * S * S, n)
    if S > 1:                                                                             # teeth: the other orientation; a tap that sees the neighbouring image
        assert (R.strip_broadcast(c["values"], 1 - columns) != c["exact"]).any()
    if B > 1:
        one = R.strip_values(c["xin"][:S * S], c["w"], c["b"], 1, S, columns)[0]
        assert np.array_equal(one[0], c["values"][0])


def test_conditions_strip_axes():
    v = list(R.STRIP_CASES.values())
    assert {s[0] for s in v} == {1, 2, 4, 8} and {s[1] for s in v} == {32, 64} and {s[2] for s in v} == {5, 26, 32}
    assert {s[3] for s in v} == {1, 3} and {s[4] for s in v} == {0, 32} and {s[5] for s in v} == {0, 6}
    assert {s[0] for s in v if s[3] == 3} == {1, 2, 4, 8}                                 # every S with neighbouring images at t = 0 and t = S - 1


@pytest.mark.parametrize("cin,M", R.CONV1X1_CASES)
def test_conditions_conv1x1_f32(cin, M):
    c = R.build_conv1x1_f32(cin, M)
    hold(c, False, (cin, M))
    assert c["x"].shape == (M * cin + 64,) and c["exact"].shape == (M, 1)


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------
STORED = ("t", "out1", "conv1_1", "conv1_2", "conv1_3", "conv1_4", "conv1_5", "slot0", "slot1", "slot2", "slot3", "slot4")


@pytest.mark.parametrize("did", [7, 8])
def test_conditions_chain(did):
    sd, enc = R.planted_state(did), R.planted_enc(did)
    assert set(np.unique(enc)) == {-1.0, 0.0, 1.0}
    for key, t in sd.items():
        if key.startswith("dense_layer.") and key.endswith("conv2.weight"):
            assert not t.any()
        if key.startswith("wsm_block.") and key.endswith(".weight"):
            rows = t.permute(1, 2, 3, 0).reshape(-1, t.shape[0]) if ".deconv1." in key else t.reshape(t.shape[0], -1)
            assert torch.equal(t, t.round()) and rows.abs().sum(1).max() <= 2 and rows.abs().sum(1).min() >= 0 and rows.abs().sum() >= rows.shape[0]
        if key.startswith("wsm_block.") and key.endswith(".bias"):
            assert set(np.unique(t.numpy())) == ({-1.0, 0.0, 1.0} if did == 7 else {0.0})
    assert set(np.unique(sd["conv1.weight"].numpy())) == set(float(v) for v in range(-4, 5)) and sd["conv1.bias"].item() == 2.0
    stages = []
    m = R.chain_f64(did, sd, enc, stages)
    assert np.array_equal(m, R.expected_map(did)) and m.shape == (2, 1, 2 ** (did - 3), 2 ** (did - 3))
    depth = 0
    for st in stages[:-1]:                                                                # (e): every stored intermediate is a bf16 number
        for key in STORED:
            v = st[key].numpy()
            assert R.is_bf16(v), (did, key)
            assert np.abs(v).max() <= 256 and np.abs(v).max() > 0, (did, key, np.abs(v).max())
        depth += 4
        if did == 8:                                                                      # zero biases: every stage at most doubles max |v|
            assert max(np.abs(st[k].numpy()).max() for k in STORED) <= 2 ** depth
    assert stages[-1]["conv1_mag"].max().item() < 2 ** 24
    assert np.array_equal(m.astype(np.float32).astype(np.float64), m) and len(np.unique(m)) > 50
    for b in range(2):                                                                    # the B = 1 maps are the B = 2 map's images
        assert np.array_equal(R.chain_f64(did, sd, enc[64 * b:64 * b + 64]), m[b:b + 1])


@pytest.mark.parametrize("what", sorted(R.mutations()))
def test_reference_has_power(what):
    """d_7, B = 1: the mutated reference gives another map"""
    change, order = R.mutations()[what]
    sd = dict(R.planted_state(7))
    change(sd)
    enc = R.planted_enc(7)[:64]
    m = R.chain_f64(7, sd, enc, slot_order=order)
    differ = m != R.expected_map(7)[:1]
    print("%s: %d of %d map entries differ" % (what, differ.sum(), differ.size))
    assert differ.any(), what
