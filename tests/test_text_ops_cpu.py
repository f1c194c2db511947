"""CPU: argument refusals of the text-side operator entry points (no HIP call is reached), the "text_rows" tuning key, and the
proof that the references and bounds of tests/_text_refs.py discriminate: the float32 restatement of every operation passes its
bound with a factor >= 4 to spare, each planted fault applied to the float64 reference misses it by a factor >= 100."""
import ctypes
import os

import pytest

torch = pytest.importorskip("torch")

import _text_refs as R          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "pnp-ovss_amd", "pnp_ovss", "libpnp_hip.so")
ERR_ARG = -22
SPARE, MISS = 4.0, 100.0


@pytest.fixture(scope="module")
def lib():
    from pnp_ovss import hip
    return hip.load_library()


def test_text_operator_entry_points_validate_arguments_without_a_gpu(lib):
    """Every refusal sits in front of the first HIP call, so it is observable on a machine without a device.  `p` stands for
    a non-null pointer that is never dereferenced (the call returns before any launch)."""
    buf = ctypes.create_string_buffer(64)
    p, n = ctypes.addressof(buf), None
    sa, sb = lib.pnp_op_text_self_attn, lib.pnp_op_text_self_attn_bwd
    assert sa(0, p, p, 513, p, p, p, 1, 513, 64, n) == ERR_ARG            # L > 512
    assert sa(1, p, p, 8, p, p, p, 1, 8, 96, n) == ERR_ARG                # H % 64 != 0
    assert sa(0, p, p, 300, p, n, n, 1, 300, 64, n) == ERR_ARG            # long form without stash or scratch
    assert sa(0, p, p, 7, p, n, n, 1, 8, 64, n) == ERR_ARG                # ld_mask < L
    for args in ((n, p, 8, p), (p, n, 8, p), (p, p, 8, n)):               # qkv, mask, ctx missing
        assert sa(0, args[0], args[1], args[2], args[3], n, n, 1, 8, 64, n) == ERR_ARG
    for B, L, H in ((0, 8, 64), (1, 0, 64), (1, 8, 0), (-1, 8, 64)):
        assert sa(0, p, p, 8, p, n, n, B, L, H, n) == ERR_ARG
        assert sb(0, p, p, p, p, p, B, L, H, n) == ERR_ARG
    assert sb(0, p, p, p, p, p, 1, 513, 64, n) == ERR_ARG
    assert sb(1, p, p, p, p, p, 1, 8, 100, n) == ERR_ARG
    for i in range(5):                                                    # each mandatory pointer of the backward
        a = [p] * 5
        a[i] = n
        assert sb(0, *a, 1, 8, 64, n) == ERR_ARG
    ln, lnb = lib.pnp_op_layernorm_ex, lib.pnp_op_layernorm_bwd
    assert ln(0, p, p, p, 1e-6, 4, 1028, p, n, n, n, n, n) == ERR_ARG     # D > 1024
    assert ln(0, p, p, p, 1e-6, 4, 770, p, n, n, n, n, n) == ERR_ARG      # D % 4 != 0
    assert ln(0, p, p, p, 1e-6, 4, 64, p, p, p, n, n, n) == ERR_ARG       # yt_lo without bf16
    assert ln(1, p, p, p, 1e-6, 4, 64, p, n, p, n, n, n) == ERR_ARG       # yt_lo without yt
    assert ln(0, p, p, p, 1e-6, 0, 64, p, n, n, n, n, n) == ERR_ARG
    assert ln(0, p, p, p, 1e-6, 4, 0, p, n, n, n, n, n) == ERR_ARG
    for i in range(3):
        a = [p] * 3
        a[i] = n
        assert ln(0, *a, 1e-6, 4, 64, p, n, n, n, n, n) == ERR_ARG
    assert lnb(0, p, p, p, p, 4, 1028, p, n, n) == ERR_ARG
    assert lnb(0, p, p, p, p, 4, 770, p, n, n) == ERR_ARG
    assert lnb(0, p, p, p, p, 0, 64, p, n, n) == ERR_ARG
    for i in range(4):
        a = [p] * 4
        a[i] = n
        assert lnb(0, *a, 4, 64, p, n, n) == ERR_ARG
    te = lib.pnp_op_text_embed
    assert te(n, 8, p, p, p, 1, 8, 64, 2, 100, n) == ERR_ARG
    assert te(p, 8, p, p, n, 1, 8, 64, 2, 100, n) == ERR_ARG
    assert te(p, 7, p, p, p, 1, 8, 64, 2, 100, n) == ERR_ARG              # ld_ids < L
    assert te(p, 8, p, p, p, 1, 8, 66, 2, 100, n) == ERR_ARG              # H % 4 != 0
    assert te(p, 8, p, p, p, 1, 8, 64, 2, 0, n) == ERR_ARG                # empty vocabulary
    assert te(p, 8, p, p, p, 0, 8, 64, 2, 100, n) == ERR_ARG
    assert lib.pnp_op_itm_head(p, p, p, n, 1, 8, 64, n) == ERR_ARG
    assert lib.pnp_op_itm_head(p, p, p, p, 0, 8, 64, n) == ERR_ARG
    assert lib.pnp_op_itm_grad_seed(p, n, 1, 8, 64, n) == ERR_ARG
    assert lib.pnp_op_itm_grad_seed(p, p, 1, 0, 64, n) == ERR_ARG
    assert lib.pnp_op_patchify(0, n, n, p, 1, 64, 4, n) == ERR_ARG
    assert lib.pnp_op_patchify(0, p, n, p, 1, 60, 4, n) == ERR_ARG        # S != 16 P
    assert lib.pnp_op_patchify(0, p, n, p, 0, 64, 4, n) == ERR_ARG
    assert lib.pnp_op_cls_rows(p, p, n, 1, 17, 64, n) == ERR_ARG
    assert lib.pnp_op_cls_rows(p, p, p, 1, 0, 64, n) == ERR_ARG


def test_text_rows_tuning_key_range(lib):
    try:
        for v in range(5):
            assert lib.pnp_set_tuning(b"text_rows", v) == 0
        assert lib.pnp_set_tuning(b"text_rows", -1) == ERR_ARG
        assert lib.pnp_set_tuning(b"text_rows", 5) == ERR_ARG
        assert lib.pnp_set_tuning(b"text_cols", 1) == ERR_ARG
    finally:
        assert lib.pnp_set_tuning(b"text_rows", 0) == 0


# ------------------------------------------------------------------------------------------ the references discriminate
def _err(a, b):
    return float((a.double() - b.double()).abs().max())


def _attn_case(L, scale, heads=4):
    kinds = ("ones", "prefix", "token0")
    qkv = R.make_qkv(3, L, heads, scale, seed=L * 10 + int(scale))
    return qkv, R.make_masks(kinds, L), R.make_dctx(3, L, heads, seed=L), heads


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("L", [5, 64, 65, 192, 193, 512])
def test_attention_float32_restatement_is_well_inside_the_bound(L, scale):
    """The formulas of attn_fwd / attn_bwd in float32 against float64: every output uses <= 1/4 of 2e-5 * max(1, max|ref|)."""
    qkv, mask, dctx, heads = _attn_case(L, scale)
    p64, c64 = R.attn_fwd(qkv, mask, heads)
    p32, c32 = R.attn_fwd(qkv, mask, heads, torch.float32)
    pst = p64.float()                                    # the stash the backward is judged on
    ref = dict(zip(("dq", "dk", "dv", "dS"), R.attn_bwd(qkv, dctx, pst, heads)))
    got = dict(zip(("dq", "dk", "dv", "dS"), R.attn_bwd(qkv, dctx, pst, heads, torch.float32)))
    ref.update(probs=p64, ctx=c64)
    got.update(probs=p32, ctx=c32)
    for name in ref:
        used = _err(got[name], ref[name]) / R.attn_bound(ref[name])
        R.measure(f"cpu/attn_f32_restatement/L{L}/s{scale:g}/{name}/fraction_of_bound", used)
        assert used * SPARE <= 1.0, (name, used)


def test_attention_formula_equals_autograd():
    for L, scale in ((5, 1.0), (65, 4.0), (193, 1.0)):
        qkv, mask, dctx, heads = _attn_case(L, scale)
        p64, _ = R.attn_fwd(qkv, mask, heads)
        dq, dk, dv, _ = R.attn_bwd(qkv, dctx, p64, heads)
        for a, b in zip((dq, dk, dv), R.attn_bwd_autograd(qkv, mask, dctx, heads)):
            assert _err(a, b) <= 1e-11 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("L", [5, 65, 512])
@pytest.mark.parametrize("fault", ["drop_last_live_key", "mask_shifted"])
def test_attention_mask_faults_miss_the_bound(fault, L):
    """A wrong mask column (one live key of one image dropped; every column shifted by one) moves probs, ctx and -- through
    the stash -- dq, dk, dv by >= 100x their bounds, at unit scale (the mildest)."""
    qkv, mask, dctx, heads = _attn_case(L, 1.0)
    p64, c64 = R.attn_fwd(qkv, mask, heads)
    pf, cf = R.attn_fwd(qkv, R.fault_mask(mask, fault), heads)
    ref = dict(zip(("dq", "dk", "dv"), R.attn_bwd(qkv, dctx, p64, heads)[:3]), probs=p64, ctx=c64)
    bad = dict(zip(("dq", "dk", "dv"), R.attn_bwd(qkv, dctx, pf, heads)[:3]), probs=pf, ctx=cf)
    for name in ref:
        over = _err(bad[name], ref[name]) / R.attn_bound(ref[name])
        R.measure(f"cpu/attn_fault/{fault}/L{L}/{name}/times_bound", over)
        assert over >= MISS, (name, over)


@pytest.mark.parametrize("L", [5, 65, 512])
@pytest.mark.parametrize("fault,outputs", [("dq_unscaled", ("dq",)), ("neighbour_probs", ("dq", "dk", "dv", "dS")),
                                           ("dv_untransposed", ("dv",))])
def test_attention_backward_faults_miss_the_bound(fault, outputs, L):
    qkv, mask, dctx, heads = _attn_case(L, 1.0)
    pst = R.attn_fwd(qkv, mask, heads)[0].float()
    names = ("dq", "dk", "dv", "dS")
    ref = dict(zip(names, R.attn_bwd(qkv, dctx, pst, heads)))
    bad = dict(zip(names, R.attn_bwd(qkv, dctx, pst, heads, fault=fault)))
    for name in names:
        over = _err(bad[name], ref[name]) / R.attn_bound(ref[name])
        if name in outputs:
            R.measure(f"cpu/attn_fault/{fault}/L{L}/{name}/times_bound", over)
            assert over >= MISS, (name, over)
        else:
            assert over == 0.0, (name, over)             # the fault is confined to the outputs it names


@pytest.mark.parametrize("L", [5, 65, 193])
def test_bf16_bound_holds_for_a_correct_rounding(L):
    """bf16 outputs: the float32 restatement rounded to bf16 (the one rounding the kernel adds to its fp32 result) stays inside
    2^-8 * max|ref| + the fp32 bound -- with little to spare, half an ulp of bf16 being up to 2^-8 of the value -- and a
    truncation instead of the rounding (up to a whole ulp) does not."""
    qkv, mask, dctx, heads = _attn_case(L, 1.0)
    qkv = qkv.to(torch.bfloat16).float()
    p64, c64 = R.attn_fwd(qkv, mask, heads)
    pst = p64.float()
    ref = dict(zip(("dq", "dk", "dv"), R.attn_bwd(qkv, dctx, pst, heads)[:3]), ctx=c64)
    got = dict(zip(("dq", "dk", "dv"), R.attn_bwd(qkv, dctx, pst, heads, torch.float32)[:3]), ctx=R.attn_fwd(qkv, mask, heads, torch.float32)[1])
    worst_trunc = 0.0
    for name in ref:
        used = _err(got[name].to(torch.bfloat16), ref[name]) / R.attn_bound_bf16(ref[name])
        R.measure(f"cpu/attn_bf16_rounding/L{L}/{name}/fraction_of_bound", used)
        assert used <= 1.0, (name, used)
        trunc = (got[name].contiguous().view(torch.int32) & -65536).view(torch.float32)
        worst_trunc = max(worst_trunc, _err(trunc, ref[name]) / R.attn_bound_bf16(ref[name]))
    assert worst_trunc > 1.0, worst_trunc


LN_SHAPES = [(130, D) for D in (4, 64, 252, 768, 1024)]


@pytest.mark.parametrize("eps", [1e-6, 1e-12])
@pytest.mark.parametrize("kind", [k for k in R.LN_KINDS if k != "constant"])
@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_float32_restatement_is_well_inside_the_bounds(rows, D, kind, eps):
    x = R.make_ln_rows(kind, rows, D, seed=D)
    w, b = R.make_ln_weights(D, seed=D)
    y, xhat, rstd = R.ln_fwd(x, w, b, eps)
    y32, xhat32, rstd32 = R.ln_fwd(x, w, b, eps, torch.float32)
    use = {"xhat": _err(xhat32, xhat) / R.ln_xhat_bound(x, xhat, rstd),
           "y": _err(y32, y) / R.ln_y_bound(x, xhat, rstd, w, y),
           "rstd": float(((rstd32.double() - rstd) / rstd).abs().max()) / R.ln_rstd_bound(x, rstd)}
    dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(D + 3))
    xh, rs = xhat.float(), rstd.float()
    use["dx"] = _err(R.ln_bwd(dy, w, xh, rs, torch.float32), R.ln_bwd(dy, w, xh, rs)) / R.ln_bwd_bound(dy, w, xh, rs)
    for name, used in use.items():
        R.measure(f"cpu/ln_f32_restatement/{kind}/D{D}/eps{eps:g}/{name}/fraction_of_bound", used)
        assert used * SPARE <= 1.0, (name, used)


def test_layernorm_constant_row_is_exact_in_float32():
    for eps in (1e-6, 1e-12):
        x = R.make_ln_rows("constant", 5, 252, seed=0)
        w, b = R.make_ln_weights(252, seed=0)
        y, xhat, rstd = R.ln_fwd(x, w, b, eps, torch.float32)
        assert torch.equal(xhat, torch.zeros_like(xhat)) and torch.equal(y, b.expand_as(y))
        assert float((rstd.double() * eps ** 0.5 - 1).abs().max()) <= 2.0 ** -21


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_layernorm_faults_miss_the_bounds(rows, D):
    w, b = R.make_ln_weights(D, seed=D)
    # the last row of a 4-row workgroup left at its input
    x = R.make_ln_rows("normal", rows, D, seed=D)
    y, xhat, rstd = R.ln_fwd(x, w, b, 1e-6)
    yb, xb, _ = R.ln_fwd(x, w, b, 1e-6, fault="last_row_of_four_unwritten")
    assert _err(yb, y) >= MISS * R.ln_y_bound(x, xhat, rstd, w, y)
    assert _err(xb, xhat) >= MISS * R.ln_xhat_bound(x, xhat, rstd) or D == 4    # D = 4: xhat of a row is x up to scale
    # one-pass variance in float32 on the 1000-offset rows
    for kind in ("offset", "tight_offset"):
        x = R.make_ln_rows(kind, rows, D, seed=D)
        y, xhat, rstd = R.ln_fwd(x, w, b, 1e-12)
        _, xb, rb = R.ln_fwd(x, w, b, 1e-12, torch.float32, fault="one_pass_variance")
        bad = torch.nan_to_num(xb.double(), nan=1e30, posinf=1e30, neginf=-1e30)         # a negative variance gives NaN
        over = _err(bad, xhat) / R.ln_xhat_bound(x, xhat, rstd)
        rbad = torch.nan_to_num(rb.double(), nan=1e30, posinf=1e30)
        rover = float(((rbad - rstd) / rstd).abs().max()) / R.ln_rstd_bound(x, rstd)
        R.measure(f"cpu/ln_fault/one_pass_variance/{kind}/D{D}/xhat/times_bound", over)
        R.measure(f"cpu/ln_fault/one_pass_variance/{kind}/D{D}/rstd/times_bound", rover)
        assert over >= MISS and rover >= MISS, (kind, over, rover)
    # mean(g * xhat) dropped from the backward
    x = R.make_ln_rows("wide", rows, D, seed=D)
    _, xhat, rstd = R.ln_fwd(x, w, b, 1e-6)
    dy = torch.randn(rows, D, generator=torch.Generator().manual_seed(D + 3))
    xh, rs = xhat.float(), rstd.float()
    over = _err(R.ln_bwd(dy, w, xh, rs, fault="xhat_term_dropped"), R.ln_bwd(dy, w, xh, rs)) / R.ln_bwd_bound(dy, w, xh, rs)
    R.measure(f"cpu/ln_fault/xhat_term_dropped/D{D}/dx/times_bound", over)
    assert over >= MISS, over


def test_itm_head_float32_restatement_is_well_inside_the_bound():
    g = torch.Generator().manual_seed(5)
    h, w, bias = torch.randn(35, 3, 768, generator=g), 0.05 * torch.randn(2, 768, generator=g), torch.randn(2, generator=g)
    ref = R.itm_head(h, w, bias)
    prod = (h[:, 0, None, :] * w[None]).view(35, 2, 12, 64)
    lanes = torch.zeros(35, 2, 64)
    for c in range(12):                                   # the kernel's order: 64 strided partial sums of H / 64 products ...
        lanes += prod[:, :, c]
    while lanes.shape[-1] > 1:                            # ... and a butterfly over the lanes
        lanes = lanes[..., ::2] + lanes[..., 1::2]
    used = float(((lanes[..., 0] + bias).double() - ref).abs().div(R.itm_bound(h, w, ref)).max())
    R.measure("cpu/itm_head_f32_lane_order/fraction_of_bound", used)
    assert used * SPARE <= 1.0, used
    seq = torch.zeros(35, 2)
    for d in range(768):                                  # the worst order, one sequential float32 sum: still inside (the
        seq += h[:, 0, d:d + 1] * w[:, d]                 # largest of these 70 logits uses 0.25, the typical one 0.1)
    used = float(((seq + bias).double() - ref).abs().div(R.itm_bound(h, w, ref)).max())
    R.measure("cpu/itm_head_f32_sequential/fraction_of_bound", used)
    assert used <= 1.0, used
    bad = R.itm_head(torch.roll(h, 1, dims=1), w, bias)   # token 1 read instead of token 0
    assert float((bad - ref).abs().div(R.itm_bound(h, w, ref)).max()) >= MISS
