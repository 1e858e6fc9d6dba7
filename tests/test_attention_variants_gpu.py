"""insv2v_attention, one kernel form at a time (csrc/attention.hip; the forms and which case runs which: tests/attention_ref.py, pinned by
tests/test_attention_variants_cpu.py through insv2v_attention_plan).

Every case: operands with poisoned gaps, the output prefilled with a NaN pattern; the call runs twice and has to give the same bits; every
element within the per-element bound of attention_ref against the float64 reference; the constant V column exact (attn_kernel) or within one
fp16 step (attn_short_kernel): the weights sum to one; every gap element of the output untouched.  Per form: a poisoned-columns case with one
head, the five extreme input families, the cross and temporal addressing kinds, a scale other than d^-1/2, and a placement check (one
problem alone against the same problem inside a launch of >= 16 workgroups).  Causal: query i does not change by a bit when the values of
every key behind it are poisoned.  SINGLE against its fall-back, the head counts of the short kernel, and the 16-head motion module."""
import functools
import math

import pytest
import torch

import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def on_gpu(name):
    """The case's operands on the device (shared: do not modify)."""
    c, data, r = R.prepared(name)
    return {k: (v.to(DEV) if v is not None else None) for k, v in data.items()}


def launch(c, g, z0=0, nz=None):
    """insv2v_attention on problems z0 .. z0 + nz - 1 of a case as a launch of its own (default: all) -> the whole output buffer, prefilled.
    z0 has to be a multiple of every `inner` unless nz == 1."""
    from insv2v import ops
    nz = c["batch"] if nz is None else nz
    out = R.o_prefill(c).to(DEV)
    ptr, args = {}, {}
    for which, buf in (("q", g["q"]), ("k", g["k"]), ("v", g["v"]), ("o", out)):
        inner, outer, step, rs = R.addr(c, "kv" if which in "kv" else which)
        assert nz == 1 or z0 % inner == 0
        off = (z0 // inner) * outer + (z0 % inner) * step + (c["o_off"] if which == "o" else 0)
        ptr[which] = buf.data_ptr() + 2 * off
        args[which] = ((inner if nz > 1 else 1, outer, step), rs)
    o_view = out[(ptr["o"] - out.data_ptr()) // 2:]
    ops.attention(ptr["q"], ptr["k"], ptr["v"], o_view, batch=nz, heads=c["heads"], head_dim=c["hd"], seq_q=c["sq"], seq_k=c["sk"], scale=c["scale"],
                  q_rs=args["q"][1], k_rs=args["k"][1], v_rs=args["v"][1], o_rs=args["o"][1], q_addr=args["q"][0], kv_addr=args["k"][0], o_addr=args["o"][0],
                  causal=c["causal"], qkv_bias=g["table"])
    return out


def check(c, r, out, what=""):
    v = R.verdict(c, r, out)
    print(f"[attn] {c['name']:34s} {R.describe(c['plan'])}: ratio {v['ratio']:.3f} gaps {v['gaps']} ones {v['ones']} {what}")
    assert v["gaps"] == 0, f"{c['name']}: {v['gaps']} gap elements of the output were written"
    assert v["ratio"] <= 1, f"{c['name']}: |out - ref| is {v['ratio']:.3g} x the bound"
    assert v["ones"] == 0, f"{c['name']}: the constant column of V is off in {v['ones']} elements: the weights do not sum to one"


@pytest.mark.parametrize("name", [c["name"] for c in R.CASES])
def test_case(name):
    c, data, r = R.prepared(name)
    g = on_gpu(name)
    a, b = launch(c, g), launch(c, g)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{name}: two launches differ"
    check(c, r, a)


@pytest.mark.parametrize("name", R.PLACEMENT)
def test_placement(name):
    """One problem is computed with the same bits wherever its workgroups land: alone, or as the last problem of a launch of >= 16 workgroups."""
    c, data, r = R.prepared(name)
    g = on_gpu(name)
    p = R.check_case_plan(c)
    assert p.grid >= 16, (name, p.grid)
    nz = c["inner"] if c["plan"][0] == R.SINGLE_REP else 1        # (REP serves the kv_inner problems of a sample in one workgroup)
    z0 = c["batch"] - nz
    whole, alone = launch(c, g), launch(c, g, z0, nz)
    torch.cuda.synchronize()
    w, a = R.real_rows(c, whole.cpu()).view(torch.int16), R.real_rows(c, alone.cpu()).view(torch.int16)
    assert torch.equal(w[z0:], a[z0:]), f"{name}: problem {z0} differs between a launch of its own and the batch"
    assert bool((a[:z0] == R.O_PREFILL).all()) and int((alone.cpu().view(torch.int16)[R.gap_mask(c)] != R.O_PREFILL).sum()) == 0


@pytest.mark.parametrize("name", R.CAUSAL)
def test_causal_ignores_later_keys(name):
    """Query i of a causal problem is bit-identical when the value of every key j > i is +-60000 (and, where the form's rounding path does not
    depend on the other queries of the wave, its K row a copy of key 0): nothing behind the diagonal enters."""
    c, data, r = R.prepared(name)
    g = on_gpu(name)
    base = R.real_rows(c, launch(c, g).cpu()).view(torch.int16)
    O, Rk, I, C = R.specs(c)["kv"]
    for i in sorted({0, 1, 14, 15, 16, 17, 31, 32, 33, 63, 64, c["sq"] - 2, c["sq"] - 1} & set(range(c["sq"]))):
        k4, v4 = g["k"].clone().view(O, Rk, I, C), g["v"].clone().view(O, Rk, I, C)
        col, row = torch.arange(C, device=DEV).view(1, 1, 1, C), torch.arange(Rk, device=DEV).view(1, Rk, 1, 1)
        v4[:, i + 1:] = (R.V_POISON * (1.0 - 2.0 * ((row + col) % 2)))[:, i + 1:].half()
        if not c["plan"][5]:       # (FOLD decides per wave whether a tile takes the exact path: other queries' scores may move query i's rounding)
            k4[:, i + 1:] = k4[:, :1]
        out = R.real_rows(c, launch(c, dict(g, k=k4.reshape(-1), v=v4.reshape(-1))).cpu()).view(torch.int16)
        assert torch.equal(out[:, :, i], base[:, :, i]), f"{name}: query {i} sees a key behind it"


@pytest.mark.parametrize("pair", [("single-q80-k77", "single-q80-k77-fallback"), ("rep-q80-k77", "rep-q80-k77-fallback")])
def test_single_against_its_fallback(pair):
    """The same problem with the output moved by 8 bytes leaves the single-tile form for <4,1>: both within the bound of the same reference."""
    (c1, d1, r1), (c2, d2, r2) = R.prepared(pair[0]), R.prepared(pair[1])
    assert c1["plan"][0] in (R.SINGLE, R.SINGLE_REP) and c2["plan"] == (R.GENERIC, 160, 4, 1, 64, 0) and c2["o_off"] == 4
    assert all(torch.equal(d1[k].view(torch.int16), d2[k].view(torch.int16)) for k in "qkv") and torch.equal(r1["ref"], r2["ref"])
    a, b = launch(c1, on_gpu(pair[0])), launch(c2, on_gpu(pair[1]))
    check(c1, r1, a, "(single tile)")
    check(c2, r2, b, "(fall-back)")
    d = (R.real_rows(c1, a.cpu()).double() - R.real_rows(c2, b.cpu()).double()).abs()
    assert bool((d <= 2 * R.bound(c1, r1)).all())


def test_bias_with_twelve_heads_is_refused():
    """The biased short kernel is compiled for <= 8 heads: the library says so, it neither runs the tables on another kernel nor drops them."""
    from insv2v import ops, _lib
    heads, hd, Fr, HW = 12, 40, 16, 4
    C = heads * hd
    assert ops.attention_short_supported(heads, hd, Fr) and not ops.attention_short_supported(heads, hd, Fr, biased=True)
    assert ops.attention_short_supported(8, hd, Fr, biased=True)
    qkv = torch.zeros((Fr * HW, 3 * C), device=DEV, dtype=torch.float16)
    out = torch.full((Fr * HW, C), 7.0, device=DEV, dtype=torch.float16)
    addr = (HW, Fr * HW * 3 * C, 3 * C)
    with pytest.raises(_lib.HipKernelError, match="unsupported"):
        ops.attention(qkv.data_ptr(), qkv.data_ptr() + 2 * C, qkv.data_ptr() + 4 * C, out, qkv_bias=torch.zeros((Fr, 3 * C), device=DEV, dtype=torch.float16),
                      batch=HW, heads=heads, head_dim=hd, seq_q=Fr, seq_k=Fr, scale=1.0, q_rs=HW * 3 * C, k_rs=HW * 3 * C, v_rs=HW * 3 * C, o_rs=HW * C,
                      q_addr=addr, kv_addr=addr, o_addr=(HW, Fr * HW * C, C))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_motion_module_with_sixteen_heads():
    """U.MotionModule at C = 1280 with 16 temporal heads over 16 frames of 2 x 3 pixels: bias tables are not for 16 heads, so q / k / v take the
    GEMM with the per-frame row bias and the unbiased short kernel - against the oracle module, within the bounds of
    test_temporal_windows_gpu.py::test_motion_module_windows_vs_oracle."""
    from insv2v import ops, synth, shapes, unet as U
    from insv2v.unet import Act
    import oracle.unet3d as ou
    C, F_, B, H, W = 1280, 16, 1, 2, 3
    mkw = dict(synth.UNET_FULL["motion_module_kwargs"], num_attention_heads=16)
    d = {}
    shapes._motion(d, "mm16", C, mkw)
    sd = synth.synth_state_dict(d)
    mm = U.MotionModule(sd, "mm16", C, 32, DEV, **mkw)
    ora = ou.MotionModule(C, 32, **mkw).eval()
    ora.load_state_dict({k[len("mm16."):]: v for k, v in sd.items()})
    x = synth.synth_input("mm16.x", (B, C, F_, H, W))
    rec = []
    ops.set_launch_recorder(rec)
    try:
        a = mm(Act(x.permute(0, 2, 3, 4, 1).reshape(B * F_ * H * W, C).to(device=DEV, dtype=torch.float16).contiguous(), B, F_, H, W), 0)
        torch.cuda.synchronize()
    finally:
        ops.set_launch_recorder(None)
    attn = [t[4] for t in rec if len(t) > 4 and t[4] and t[4][0] == "attn"]
    assert len(attn) == 2 and all(t[1:] == (B * H * W, 16, 80, F_, F_) for t in attn), attn
    out = a.t.float().reshape(B, F_, H, W, C).permute(0, 4, 1, 2, 3).cpu()
    with torch.no_grad():
        ref = ora(x.float(), 0)
    rms = ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    mx = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"[parity] motion module C={C} heads=16 F={F_}: rel-rms {rms:.3e}  max-abs/max-ref {mx:.3e}")
    assert math.isfinite(rms) and rms <= 1e-2 and mx <= 4e-2, (rms, mx)
    assert (out - x).abs().max() > 1e-2   # the temporal path is live
