"""ViT glue and backward kernels (csrc/vit_ops.hip, x3.hip, pass_tree.hip), entry point by entry point, against float64 references
computed from exactly the bf16 / fp32 operands each kernel reads: the bounds below measure only the kernel's own arithmetic and output
rounding.  Every comparison is over the full output tensor, element by element; outputs that accumulate start from nonzero values, and
memory a kernel must not write holds a finite sentinel that is checked bit for bit.

Bounds: u = 2^-24 (fp32 unit roundoff).  An fp32 sum whose longest chain of sequential roundings is L is within L * u * sum|terms| of the
exact sum; an accumulating output adds its prior value to the terms.  Any order of summation of n terms has L <= n - 1, which covers
atomics and MFMA trees.  A product of two fp32 values adds u of itself, so each term carries its own (1 + k u) factor, folded into L.  A
bf16 output of an exact fp32 value is round-to-nearest-even, which torch's cast reproduces bit for bit; pure copies and gathers must be
bit-identical.  L is stated next to each test from the kernel's loop structure.

The last three tests replay a real ViT backward (ViT-S/2 at 32 x 32, in bf16 and in bf16x3, and ViT-S/16 at 224 x 224), capture the operands
of the LayerNorm and patch-embedding launches, and recompute the gradient block's LayerNorm, patch-embedding and head gradients in float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vit_ref as V                    # noqa: E402
from semireward_amd import ops                     # noqa: E402
from semireward_amd.nets import vit                # noqa: E402
from semireward_amd.utils import synth             # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
SENT = 3.0e4                                       # finite sentinel in memory a kernel must leave alone
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
RPS = 257                                          # rows per image of ViT-S/2 at 32 x 32 (256 patches + cls)


def cdiv(a, b):
    return -(-a // b)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(shape, g, scale=1.0, dtype=f32):
    return (torch.randn(shape, generator=g, dtype=f64) * scale).to(dtype).to(DEV)


def check(name, got, ref, tol):
    """|got - ref| <= tol element by element (float64); prints the largest deviation and its share of the bound."""
    got, ref = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=f64, device=ref.device).expand_as(ref)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), name
    ratio = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("DEV %-44s max|err| %.3e  max err/tol %.3f" % (name, float(err.max()) if err.numel() else 0.0, ratio))
    bad = err > tol
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside the bound; first at flat %d: got %.8g ref %.8g tol %.3g" % (
            name, int(bad.sum()), err.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(tol.reshape(-1)[i])))


def same_bits(name, got, ref):
    """bit-for-bit equality (compares the raw words, so -0.0 / 0.0 and NaN payloads count)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    w = {4: torch.int32, 2: torch.int16}[got.element_size()]
    a, b = got.contiguous().view(w), ref.contiguous().view(w)
    if not torch.equal(a, b):
        bad = (a != b).reshape(-1)
        i = int(bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at flat %d: got %r ref %r" % (
            name, int(bad.sum()), bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i])))


def patches64(img, idx, ps):
    """[n_img, C, HW, HW] gathered through idx -> [B, Np, C * ps * ps], (c, i, j) minor order (float64, exact)"""
    sel = img.double()[idx.long()] if idx is not None else img.double()
    return V.patchify(sel, ps)


def droppath_table(g, depth, cols, keep=0.8):
    """[depth, 2, cols] per-sample DropPath factors drawn from {0, 1, 1 / keep} (fp32)"""
    v = torch.tensor([0.0, 1.0, 1.0 / keep], dtype=f32)[torch.randint(0, 3, (depth, 2, cols), generator=g)]
    return v.to(DEV)


# ---- LayerNorm backward with partial copies -----------------------------------------------------------------------------------------
# dx += rstd (gy - mean(gy) - xhat mean(gy xhat)), gy = dy gamma, xhat = (x - mean) rstd from the fp32 mean / rstd operands;
# part[w % n_rep] += (sum dy xhat, sum dy) over the rows of workgroup w (4 * RPW rows; RPW = 2 below 16384 rows, else 8);
# out = cast(row_scale[row / rps] * dx_after) -- one fp32 multiply, one round-to-nearest cast.
def ln_inputs(M, D, seed):
    g = gen(seed)
    x = (torch.randn(M, D, generator=g, dtype=f64) * 2.0 + 0.5)
    mean = x.mean(-1).float()
    rstd = (1.0 / (x.var(-1, unbiased=False) + 1e-6).sqrt()).float()
    x = x.float()
    gamma = (1.0 + 0.3 * torch.randn(D, generator=g, dtype=f64)).float()
    dy = torch.randn(M, D, generator=g, dtype=f64)
    dx0 = torch.randn(M, D, generator=g, dtype=f64).float()
    return [t.to(DEV) for t in (x, mean, rstd, gamma, dy, dx0)]


def ln_bwd_ref(dy, x, mean, rstd, gamma):
    """float64 (ddx, per-row dy * xhat, per-row dy, tol of ddx) from the kernel's operands"""
    dy, x, mu, rs, ga = dy.double(), x.double(), mean.double()[:, None], rstd.double()[:, None], gamma.double()
    D = x.shape[1]
    xh = (x - mu) * rs
    gy = dy * ga
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    ddx = rs * (gy - c1 - xh * c2)
    # c1, c2: each lane sums 2 NV = D / 64 terms, then a 6-level wave tree, then the 1 / D product; gy, xhat carry 2 u each
    L = D // 64 + 6 + 4
    a1, a2 = gy.abs().mean(-1, keepdim=True), (gy * xh).abs().mean(-1, keepdim=True)
    tol = rs * (L * U * (a1 + xh.abs() * a2) + 4 * U * (gy.abs() + c1.abs() + (xh * c2).abs())) + U * ddx.abs()
    return ddx, dy * xh, dy, tol


LN_D = [128, 384, 512, 768]
LN_M = [7, 16 * RPS, 64 * RPS + 3]          # below the 16384-row switch (one partial workgroup / 514 full ones), above it with a ragged tail


@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("f32_dy", [False, True], ids=["bf16", "f32"])
def test_layernorm_bwd_part(f32_dy, M, D):
    x, mean, rstd, gamma, dy64, dx0 = ln_inputs(M, D, 100 * D + M % 97 + int(f32_dy))
    dy = dy64.float() if f32_dy else dy64.to(bf16)
    ddx, gterm, bterm, tol_dx = ln_bwd_ref(dy, x, mean, rstd, gamma)
    RPW = 2 if M < 16384 else 8
    nwg = cdiv(M, 4 * RPW)
    wg_of_row = torch.arange(M, device=DEV) // (4 * RPW)
    nsamp = cdiv(M, RPS)
    g = gen(7 + M)
    col0 = 5
    table = droppath_table(g, 12, col0 + nsamp + 3)             # [depth, 2, B] with the images of this launch at columns col0 ..
    blk, half = 7, 1
    # neighbouring images get different factors (1 / keep, 0, 1, ...): a row given its neighbour's factor changes its output bits
    table[blk, half, col0:col0 + nsamp] = torch.tensor([1.25, 0.0, 1.0], device=DEV).repeat(cdiv(nsamp, 3))[:nsamp]
    scale = ops.RawRows(table, blk * table.stride(0) + half * table.stride(1) + col0)
    sc_row = table[blk, half, col0:col0 + nsamp].repeat_interleave(RPS)[:M][:, None]
    assert M < 3 * RPS or (float(sc_row.min()) == 0.0 and float(sc_row.max()) > 1.0)
    fn = ops.layernorm_bwd_part_f32 if f32_dy else ops.layernorm_bwd_part
    out_t = f32 if f32_dy else bf16
    for n_rep, row_scale, with_out in [(16, scale, True), (1, None, True), (16, None, False)]:
        part0 = randn((n_rep, 2, D), gen(n_rep + D))
        part, dx = part0.clone(), dx0.clone()
        out = torch.full((M, D), SENT, dtype=out_t, device=DEV) if with_out else None
        fn(dy, x, mean, rstd, gamma, dx, part, n_rep, out, row_scale, RPS if row_scale is not None else 0, M, D)
        tag = "%s M=%d D=%d n_rep=%d%s" % ("f32" if f32_dy else "bf16", M, D, n_rep, " scaled" if row_scale is not None else "")
        check("ln dx " + tag, dx, dx0.double() + ddx, tol_dx + U * (dx0.double() + ddx).abs())
        # every copy holds exactly the rows of its workgroups: chain = RPW rows per lane, 3 wave adds, ceil(nwg / n_rep) atomics, 3 u per term
        copy = (wg_of_row % n_rep)
        ref = torch.zeros(n_rep, 2, D, dtype=f64, device=DEV)
        mag = torch.zeros(n_rep, 2, D, dtype=f64, device=DEV)
        ref[:, 0].index_add_(0, copy, gterm)
        ref[:, 1].index_add_(0, copy, bterm)
        mag[:, 0].index_add_(0, copy, gterm.abs())
        mag[:, 1].index_add_(0, copy, bterm.abs())
        L = RPW + 3 + cdiv(nwg, n_rep) + 3
        check("ln part " + tag, part.double() - part0.double(), ref, L * U * (mag + part0.double().abs()))
        if with_out:
            sc = sc_row if row_scale is not None else torch.ones(M, 1, device=DEV)
            same_bits("ln out " + tag, out, (dx * sc).to(out_t))


def test_ln_grad_reduce_folds_interleaved_copies(vit_s2):
    """24 LayerNorms x 16 copies folded into the views of ONE flat gradient block in vit.py's order (norm1, norm2 of block 0, 1, ..)."""
    model = vit_s2
    D, n_rep = 384, vit.LN_REP
    names = [("blocks.%d.norm%d.weight" % (i, j), "blocks.%d.norm%d.bias" % (i, j)) for i in range(12) for j in (1, 2)]
    g = gen(3)
    model.grad.copy_(torch.randn(model.grad.numel(), generator=g, dtype=f64).float().to(DEV))
    prior = model.grad.clone()
    pairs = [(model.p(a, model.grad), model.p(b, model.grad)) for a, b in names]
    desc = ops.make_ln_reduce_desc(pairs, DEV)
    part = randn((len(names), n_rep, 2, D), g)
    part0 = part.clone()
    ops.ln_grad_reduce(desc, part, len(names), n_rep, D)
    torch.cuda.synchronize()
    touched = torch.zeros(model.grad.numel(), dtype=torch.bool, device=DEV)
    for k, (a, b) in enumerate(names):
        for h, n in enumerate((a, b)):
            o = model.offsets[n][0]
            s = part0[k, :, h].double()
            # acc = sum of n_rep copies in order, then one add into the block
            check("reduce %s" % n, model.grad[o:o + D], prior[o:o + D].double() + s.sum(0),
                  (n_rep + 1) * U * (s.abs().sum(0) + prior[o:o + D].double().abs()))
            touched[o:o + D] = True
    same_bits("reduce: the rest of the block", model.grad[~touched], prior[~touched])
    assert int(torch.count_nonzero(part)) == 0, "the copies are cleared for the next step"
    after = model.grad.clone()
    ops.ln_grad_reduce(desc, part, len(names), n_rep, D)
    same_bits("reduce: a second call adds nothing", model.grad, after)
    model.zero_grad()


# ---- patch embedding, small patches (K = C ps^2 <= 64): the two-stage fixed-order backward -------------------------------------------------
PE_WS = [(16, 3, 32, 2, 384),       # the headline: 8 full 32-token chunks per image
         (5, 3, 30, 2, 384),        # 225 patches: the last chunk holds 1 token
         (4, 3, 30, 3, 128),        # K = 27: the second 16-tap register block is partial
         (3, 4, 32, 4, 192),        # K = 64, the limit
         (2, 1, 32, 8, 1024)]       # K = 64 with D = 1024 (one thread per feature)


@pytest.mark.parametrize("B,C,HW,ps,D", PE_WS)
def test_patch_embed_bwd_ws(B, C, HW, ps, D):
    g = gen(B * 1000 + HW * 10 + ps)
    gw, K = HW // ps, C * ps * ps
    Np, N = gw * gw, gw * gw + 1
    n_img = B + 3
    img = randn((n_img, C, HW, HW), g)
    idx = torch.tensor([(7 * b + 3) % n_img for b in range(B)], dtype=torch.int32)
    if B > 1:
        idx[B - 1] = idx[0]                                      # a repeated image
    idx = idx.to(DEV)
    dx = randn((B, N, D), g)
    dW0, db0, dc0, dp0 = randn((D, K), g), randn((D,), g), randn((D,), g), randn((N, D), g)
    nws = ops.patch_embed_bwd_ws_floats(B, C, HW, ps, D)
    nch = cdiv(Np, 32)
    assert nws == nch * B * (K + 1) * D
    outs = []
    for fill in (float("nan"), -7.0):                            # every workspace word is written before it is read
        ws = torch.full((nws,), fill, dtype=f32, device=DEV)
        dW, db, dc, dp = dW0.clone(), db0.clone(), dc0.clone(), dp0.clone()
        ops.patch_embed_bwd_ws(dx, img, idx, dW, db, dc, dp, ws, B, C, HW, ps, D)
        outs.append((dW, db, dc, dp))
    pt = patches64(img, idx, ps)                                 # [B, Np, K]
    gt = dx.double()[:, 1:]                                      # [B, Np, D]
    # dW, db: 32 tokens per chunk, then the fold over nch * B workgroups in order, then the add into the prior; 1 u for the product
    L = 32 + nch * B + 2
    refW = torch.einsum("bpd,bpk->dk", gt, pt)
    magW = torch.einsum("bpd,bpk->dk", gt.abs(), pt.abs())
    dW, db, dc, dp = outs[0]
    check("pe_ws dWp", dW, dW0.double() + refW, L * U * (magW + dW0.double().abs()))
    check("pe_ws dbp", db, db0.double() + gt.sum((0, 1)), L * U * (gt.abs().sum((0, 1)) + db0.double().abs()))
    # dpos, dcls: B images in order, then the add
    check("pe_ws dpos", dp, dp0.double() + dx.double().sum(0), (B + 1) * U * (dx.double().abs().sum(0) + dp0.double().abs()))
    check("pe_ws dcls", dc, dc0.double() + dx.double()[:, 0].sum(0), (B + 1) * U * (dx.double()[:, 0].abs().sum(0) + dc0.double().abs()))
    for a, b, n in zip(outs[0], outs[1], ("dWp", "dbp", "dcls", "dpos")):
        same_bits("pe_ws fixed order: " + n, b, a)


# ---- patch embedding, large patches (K > 64): im2col -> GEMM -> assemble; backward operands -----------------------------------------------
@pytest.mark.parametrize("HW", [96, 224])
def test_patch_im2col(HW):
    ps, C, B = 16, 3, 3
    g = gen(HW)
    img = randn((4, C, HW, HW), g)
    idx = torch.tensor([2, 0, 2], dtype=torch.int32, device=DEV)
    Np, K = (HW // ps) ** 2, C * ps * ps
    ref = V.patchify(img[idx.long()], ps).reshape(B * Np, K)     # an exact gather in fp32
    col = torch.full((B * Np, K), float("nan"), dtype=bf16, device=DEV)
    ops.patch_im2col(img, idx, col, B, C, HW, ps)
    same_bits("im2col bf16", col, ref.to(bf16))
    col32 = torch.full((B * Np, K), float("nan"), dtype=f32, device=DEV)
    ops.patch_im2col_f32(img, idx, col32, B, C, HW, ps)
    same_bits("im2col f32", col32, ref)


@pytest.mark.parametrize("Np,D", [(36, 192), (196, 384), (36, 768)])
def test_patch_assemble(Np, D):
    g = gen(Np + D)
    B, N = 3, Np + 1
    tok, bp, cls, pos = randn((B * Np, D), g), randn((D,), g), randn((D,), g), randn((N, D), g)
    x = torch.full((B + 1, N, D), SENT, device=DEV)
    ops.patch_assemble(tok, bp, cls, pos, x, B, Np, D)
    ref = torch.empty(B, N, D, dtype=f64, device=DEV)
    ref[:, 0] = cls.double() + pos.double()[0]
    ref[:, 1:] = tok.double().reshape(B, Np, D) + bp.double() + pos.double()[1:]
    mag = torch.empty_like(ref)
    mag[:, 0] = cls.double().abs() + pos.double()[0].abs()
    mag[:, 1:] = tok.double().abs().reshape(B, Np, D) + bp.double().abs() + pos.double()[1:].abs()
    check("assemble", x[:B], ref, 2.001 * U * mag)               # (tok + bp) + pos: two roundings
    assert bool((x[B] == SENT).all()), "assemble wrote past the last image"


@pytest.mark.parametrize("D", [384, 768])                        # D < 512 and D >= 512 take different workgroup sizes
@pytest.mark.parametrize("as_f32", [False, True], ids=["bf16", "f32"])
def test_patch_grad_operands(as_f32, D):
    g = gen(D + int(as_f32))
    B, Np = 3, 196
    N = Np + 1
    dx = randn((B, N, D), g)
    dp0, dc0 = randn((N, D), g), randn((D,), g)
    dp, dc = dp0.clone(), dc0.clone()
    t = f32 if as_f32 else bf16
    dxt = torch.full((B * Np, D), float("nan"), dtype=t, device=DEV)
    (ops.patch_grad_operands_f32 if as_f32 else ops.patch_grad_operands)(dx, dxt, dp, dc, B, Np, D)
    same_bits("grad operands dx_tok", dxt, dx[:, 1:].reshape(B * Np, D).to(t))
    check("grad operands dpos", dp, dp0.double() + dx.double().sum(0), (B + 1) * U * (dx.double().abs().sum(0) + dp0.double().abs()))
    check("grad operands dcls", dc, dc0.double() + dx.double()[:, 0].sum(0),
          (B + 1) * U * (dx.double()[:, 0].abs().sum(0) + dc0.double().abs()))


@pytest.mark.parametrize("M", [16 * RPS, 16 * RPS + 5])
@pytest.mark.parametrize("scaled", [True, False])
def test_scale_rows_f32(M, scaled):
    D = 384
    g = gen(M + int(scaled))
    x = randn((M, D), g)
    nsamp = cdiv(M, RPS)
    table = droppath_table(g, 12, 2 + nsamp + 4)
    out = torch.full((M, D), float("nan"), device=DEV)
    if scaled:
        ops.scale_rows_f32(x, ops.RawRows(table, 11 * table.stride(0) + 1 * table.stride(1) + 2), RPS, out, M, D)
        sc = table[11, 1, 2:2 + nsamp].repeat_interleave(RPS)[:M][:, None]
        same_bits("scale_rows_f32", out, x * sc)
    else:
        ops.scale_rows_f32(x, None, 0, out, M, D)
        same_bits("scale_rows_f32 unscaled", out, x)


# ---- classification head backward, in the two split forms the model calls -----------------------------------------------------------
@pytest.mark.parametrize("B,N,D,C", [(16, 257, 384, 100), (7, 17, 128, 10), (3, 5, 768, 1000)])
def test_cls_head_bwd_split(B, N, D, C):
    g = gen(B * N + C)
    dl, Wh, gamma = randn((B, C), g), randn((C, D), g, D ** -0.5), 1.0 + randn((D,), g, 0.3)
    feat, xhat, rstd = randn((B, D), g), randn((B, D), g), 1.0 + randn((B,), g).abs()
    dgn0, dbn0, dWh0, dbh0 = randn((D,), g), randn((D,), g), randn((C, D), g), randn((C,), g)
    dx = torch.full((B, N, D), SENT, device=DEV)                 # row 0 of each image is assigned, the rest stays
    dgn, dbn, dWh, dbh = dgn0.clone(), dbn0.clone(), dWh0.clone(), dbh0.clone()
    # backward_rows: dx of the cls rows and the final norm's affine gradients
    ops.cls_head_bwd(dl, Wh, gamma, None, xhat, rstd, dx, None, None, dgn, dbn, B, N, D, C)
    same_bits("cls_head dWh untouched by the rows form", dWh, dWh0)
    # backward_finish: the head's weight and bias gradients
    ops.cls_head_bwd(dl, None, None, feat, None, None, None, dWh, dbh, None, None, B, N, D, C)
    d64, W64, g64, xh, rs = dl.double(), Wh.double(), gamma.double(), xhat.double(), rstd.double()[:, None]
    df = d64 @ W64
    e_df = (C + 1) * U * (d64.abs() @ W64.abs())                 # C-term chain per feature
    gy = df * g64
    e_gy = g64.abs() * e_df + U * gy.abs()
    Lb = cdiv(D, 256) + 6 + 4 + 1                                # per-thread terms, wave tree, 4 waves, the 1 / D product
    c1, c2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    e_c1 = e_gy.mean(-1, keepdim=True) + Lb * U * gy.abs().mean(-1, keepdim=True)
    e_c2 = (e_gy * xh.abs()).mean(-1, keepdim=True) + (Lb + 1) * U * (gy * xh).abs().mean(-1, keepdim=True)
    ref = rs * (gy - c1 - xh * c2)
    tol = rs * (e_gy + e_c1 + xh.abs() * e_c2 + 3 * U * (gy.abs() + c1.abs() + (xh * c2).abs())) + U * ref.abs()
    check("cls_head dx", dx[:, 0], ref, tol)
    assert bool((dx[:, 1:] == SENT).all()), "cls_head_bwd wrote a row other than the cls row"
    Lg = B + 2
    check("cls_head dgamma", dgn, dgn0.double() + (df * xh).sum(0),
          (xh.abs() * e_df).sum(0) + Lg * U * ((df * xh).abs().sum(0) + dgn0.double().abs()))
    check("cls_head dbeta", dbn, dbn0.double() + df.sum(0), e_df.sum(0) + Lg * U * (df.abs().sum(0) + dbn0.double().abs()))
    check("cls_head dWh", dWh, dWh0.double() + d64.t() @ feat.double(), Lg * U * (d64.abs().t() @ feat.double().abs() + dWh0.double().abs()))
    check("cls_head dbh", dbh, dbh0.double() + d64.sum(0), Lg * U * (d64.abs().sum(0) + dbh0.double().abs()))


# ---- pass-prefix tree copies --------------------------------------------------------------------------------------------------------
def _offset_rows(rows, width, offset_words, g, dtype=f32, tail=64):
    """a [rows, width] table at ``offset_words`` elements into a buffer of random words that runs ``tail`` elements past it; returns
    (table, buffer)"""
    buf = randn((offset_words + rows * width + tail,), g, 1.0, dtype)
    return buf[offset_words:offset_words + rows * width].view(rows, width), buf


@pytest.mark.parametrize("rpn,D,offset,with_ln", [(257, 384, 0, True), (257, 384, 0, False), (257, 384, 1, True), (3, 10, 0, True)],
                         ids=["16B-ln", "16B", "offset4B-ln", "narrow4B-ln"])
def test_vit_fork(rpn, D, offset, with_ln):
    g = gen(rpn * D + offset)
    dst0, n_new, slack = 5, 5, 2
    nodes = dst0 + n_new + slack
    x, xbuf = _offset_rows(nodes, rpn * D, offset, g)
    ln, lbuf = _offset_rows(nodes, rpn * D, 2 * offset, g, bf16) if with_ln else (None, None)
    parent = torch.tensor([2, 0, -1, dst0, 4], dtype=torch.int32, device=DEV)  # a negative and a >= dst0 parent copy nothing
    x0, l0 = xbuf.clone(), (lbuf.clone() if with_ln else None)
    ops.vit_fork(x.view(nodes, rpn, D), ln.view(nodes, rpn, D) if with_ln else None, parent, n_new, dst0, rpn, D)
    for buf, ref0, tab in ([(xbuf, x0, x)] + ([(lbuf, l0, ln)] if with_ln else [])):
        want = ref0.clone()
        off = tab.data_ptr() - buf.data_ptr()
        wt = want[off // buf.element_size():off // buf.element_size() + tab.numel()].view(tab.shape)
        for k, p in enumerate(parent.tolist()):
            if 0 <= p < dst0:
                wt[dst0 + k] = wt[p]
        same_bits("fork %s" % tab.dtype, buf, want)


@pytest.mark.parametrize("C,offset", [(10, 0), (100, 0), (100, 1)], ids=["logits40B", "logits400B-16B", "logits400B-offset4B"])
def test_vit_fanout(C, offset):
    D = 384
    g = gen(C + offset)
    n_nodes, rows_l, rows_f = 6, 24, 20                          # the feature table is the shorter one
    node_logits, node_feat = randn((n_nodes, C), g), randn((n_nodes, D), g)
    la, lbuf = _offset_rows(rows_l, C, offset, g)
    fa, fbuf = _offset_rows(rows_f, D, offset, g, tail=(rows_l - rows_f + 1) * D)    # a row >= rows_f would land in the buffer's tail
    col_node = torch.tensor([0, 5, 3, -1, 6, 2, 1, 4, 1], dtype=torch.int32, device=DEV)     # nodes -1 and n_nodes copy nothing,
    col_rows = torch.tensor([3, 0, 19, 7, 8, -1, 20, 22, 11], dtype=torch.int64, device=DEV)  # nor do rows -1 and >= rows_f
    l0, f0 = lbuf.clone(), fbuf.clone()
    ops.vit_fanout(node_logits, node_feat, n_nodes, col_node, col_rows, col_node.numel(), la, fa, C, D)
    wl, wf = l0.clone(), f0.clone()
    wlt, wft = wl[offset:offset + la.numel()].view(rows_l, C), wf[offset:offset + fa.numel()].view(rows_f, D)
    valid = 0
    for n, r in zip(col_node.tolist(), col_rows.tolist()):
        if 0 <= n < n_nodes and 0 <= r < min(rows_l, rows_f):
            wlt[r], wft[r] = node_logits[n], node_feat[n]
            valid += 1
    assert valid == 4
    same_bits("fanout logits", lbuf, wl)
    same_bits("fanout feat", fbuf, wf)


# ---- replays of a real backward ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vit_s2():
    cfg = V.VitCfg(num_classes=100, **V.VIT_SMALL_P2_32)
    model = vit.vit_small_patch2_32(num_classes=100, device=DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(V.param_shapes(cfg), 11).items()})
    model.cfg_ref = cfg
    return model


class _Capture:
    """Wraps one ops entry point: clones the arguments at ``inputs`` before the call and at ``outputs`` after it (later launches may
    overwrite both), keeps the rest as given."""

    def __init__(self, monkeypatch, name, inputs=(), outputs=()):
        self.calls, fn = [], getattr(ops, name)

        def wrapped(*a):
            a = list(a)
            for i in inputs:
                a[i] = a[i].clone() if a[i] is not None else None
            r = fn(*a)
            for i in outputs:
                a[i] = a[i].clone()
            self.calls.append(a)
            return r
        monkeypatch.setattr(ops, name, wrapped)


def _check_ln_grads(model, calls, tag):
    """every norm1 / norm2 dgamma, dbeta of the gradient block against float64 sums from the operands its launch read"""
    cfg = model.cfg
    by_gamma = {model.p("blocks.%d.norm%d.weight" % (i, j)).data_ptr(): (i, j) for i in range(cfg.depth) for j in (1, 2)}
    seen = set()
    for a in calls:
        dy, x, mean, rstd, gamma, n_rep, M, D = a[0], a[1], a[2], a[3], a[4], a[7], a[11], a[12]
        i, j = by_gamma[gamma.data_ptr()]
        seen.add((i, j))
        _, gterm, bterm, _ = ln_bwd_ref(dy, x, mean, rstd, gamma)
        RPW = 2 if M < 16384 else 8
        # RPW rows per lane, 3 wave adds, ceil(nwg / n_rep) atomics per copy, n_rep copies folded, one add into the block, 3 u per term
        L = RPW + 3 + cdiv(cdiv(M, 4 * RPW), n_rep) + n_rep + 1 + 3
        gw, gb = model.view("blocks.%d.norm%d.weight" % (i, j), model.grad), model.view("blocks.%d.norm%d.bias" % (i, j), model.grad)
        check("%s blocks.%d.norm%d dgamma" % (tag, i, j), gw, gterm.sum(0), L * U * gterm.abs().sum(0))
        check("%s blocks.%d.norm%d dbeta" % (tag, i, j), gb, bterm.sum(0), L * U * bterm.abs().sum(0))
    assert len(seen) == 2 * cfg.depth == len(calls), (len(seen), len(calls))


def _check_pos_cls(model, dx, B, tag):
    """dpos, dcls of a zeroed block from the dx the patch-embedding backward read: B images in order"""
    dx = dx.double().reshape(B, model.cfg.num_tokens, -1)
    check(tag + " dpos", model.view("pos_embed", model.grad)[0], dx.sum(0), (B + 1) * U * dx.abs().sum(0))
    check(tag + " dcls", model.view("cls_token", model.grad).reshape(-1), dx[:, 0].sum(0), (B + 1) * U * dx[:, 0].abs().sum(0))


def _check_head(model, ctx, dl, tag):
    B = dl.shape[0]
    d64, f64_ = dl.double(), ctx.feat.double()
    check(tag + " head dW", model.view("head.weight", model.grad), d64.t() @ f64_, (B + 1) * U * (d64.abs().t() @ f64_.abs()))
    check(tag + " head db", model.view("head.bias", model.grad), d64.sum(0), (B + 1) * U * d64.abs().sum(0))


def _forward_backward(model, img, idx, dp, precision):
    B = idx.numel()
    C = model.cfg.num_classes
    lg, _, ctx = model.forward_features(img, idx, dp, save=True, precision=precision)
    y = torch.randint(0, C, (B,), generator=gen(5)).to(DEV)
    w = torch.rand(B, generator=gen(6)).to(DEV)
    loss, dl = torch.empty(1, device=DEV), torch.empty(B, C, device=DEV)
    ops.masked_ce(lg, y, w, None, 1.0, loss, dl, B, C)
    model.zero_grad()
    model.backward(ctx, dl)
    torch.cuda.synchronize()
    return ctx, dl


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_vit_s2_backward_replay(vit_s2, precision, monkeypatch):
    """The headline shape: 16 images (4112 rows: 514 LayerNorm workgroups into 16 copies), an injected DropPath table of 0 and 1 / keep."""
    model = vit_s2
    cfg = model.cfg_ref
    B, n_img = 16, 20
    g = gen(17)
    img = randn((n_img, 3, 32, 32), g)
    idx = torch.tensor([(3 * b + 1) % n_img for b in range(B)], dtype=torch.int32)
    idx[5] = idx[2]
    idx = idx.to(DEV)
    dp = torch.from_numpy(synth.synth_droppath(23, V.drop_path_probs(cfg), B)).to(DEV)
    assert float(dp.min()) == 0.0 and float(dp.max()) > 1.0
    ln = _Capture(monkeypatch, "layernorm_bwd_part_f32" if precision == "bf16x3" else "layernorm_bwd_part", inputs=(0, 1, 2, 3))
    pe = _Capture(monkeypatch, "patch_embed_bwd_ws", inputs=(0,))
    model.grad_rows_precision = precision
    try:
        ctx, dl = _forward_backward(model, img, idx, dp, precision)
    finally:
        model.grad_rows_precision = "bf16"
    _check_ln_grads(model, ln.calls, precision)
    assert len(pe.calls) == 1
    a = pe.calls[0]
    dx, img_, idx_, Bc, C, HW, ps, D = a[0], a[1], a[2], a[8], a[9], a[10], a[11], a[12]
    assert Bc == B and idx_ is not None and torch.equal(idx_, idx)
    pt = patches64(img_, idx_, ps)
    gt = dx.double().reshape(B, -1, D)[:, 1:]
    nch = cdiv(pt.shape[1], 32)
    L = 32 + nch * B + 2
    check(precision + " dWp", model.view("patch_embed.proj.weight", model.grad).reshape(D, -1), torch.einsum("bpd,bpk->dk", gt, pt),
          L * U * torch.einsum("bpd,bpk->dk", gt.abs(), pt.abs()))
    check(precision + " dbp", model.view("patch_embed.proj.bias", model.grad), gt.sum((0, 1)), L * U * gt.abs().sum((0, 1)))
    _check_pos_cls(model, dx, B, precision)
    _check_head(model, ctx, dl, precision)
    model.zero_grad()


def test_vit_s16_224_backward_replay(monkeypatch):
    """K = 768: im2col -> patch_grad_operands -> the grouped TN product for the filter gradient, 2 images."""
    cfg = V.VitCfg(num_classes=100, **V.VIT_SMALL_P16_224)
    model = vit.vit_small_patch16_224(num_classes=100, device=DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.synth_params(V.param_shapes(cfg), 12).items()})
    B = 2
    g = gen(19)
    img = randn((3, 3, 224, 224), g)
    idx = torch.tensor([2, 0], dtype=torch.int32, device=DEV)
    dp = torch.from_numpy(synth.synth_droppath(29, V.drop_path_probs(cfg), B)).to(DEV)
    ln = _Capture(monkeypatch, "layernorm_bwd_part", inputs=(0, 1, 2, 3))
    col = _Capture(monkeypatch, "patch_im2col", outputs=(2,))
    gop = _Capture(monkeypatch, "patch_grad_operands", inputs=(0,), outputs=(1,))
    ctx, dl = _forward_backward(model, img, idx, dp, "bf16")
    _check_ln_grads(model, ln.calls, "p16")
    col_bwd = col.calls[-1][2]                                   # the backward's im2col (the forward's comes first)
    assert torch.equal(col.calls[-1][1], idx) and len(gop.calls) == 1
    dx, dxt = gop.calls[0][0], gop.calls[0][1]
    D, Np = cfg.embed_dim, (224 // 16) ** 2
    same_bits("p16 im2col operand", col_bwd, V.patchify(img[idx.long()], 16).reshape(B * Np, -1).to(bf16))
    same_bits("p16 dx_tok operand", dxt, dx.reshape(B, Np + 1, D)[:, 1:].reshape(B * Np, D).to(bf16))
    a, c = dxt.double(), col_bwd.double()
    L = B * Np + 2                                              # any order over the B * Np rows, then the add into the zeroed block
    check("p16 dWp", model.view("patch_embed.proj.weight", model.grad).reshape(D, -1), a.t() @ c, L * U * (a.abs().t() @ c.abs()))
    check("p16 dbp", model.view("patch_embed.proj.bias", model.grad), a.sum(0), L * U * a.abs().sum(0))
    _check_pos_cls(model, dx, B, "p16")
    _check_head(model, ctx, dl, "p16")
