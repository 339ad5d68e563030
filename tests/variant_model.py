"""The kernel instantiations behind the 1x1-GEMM and the dense 3x3-conv entry points, and the dispatches that pick them,
restated in Python.  Pure host code: tests/test_planner_cpu.py sweeps the launch planners against it,
tests/test_gpu_gemm_variants.py and tests/test_gpu_conv_variants.py run a case on every entry, and
tests/test_gpu_launch_replay.py holds production's launches against both.

1x1 GEMM: irm_gemm1x1_f32 and irm_gemm1x1_f16x3_f32 both go through gemm_entry (csrc/gemm_pw.hip), which picks one of 78
instantiations of gemm_ring_kernel, gemm_pw_kernel and gemm_xres_kernel: VARIANTS, expected_variant().

3x3 conv: irm_conv3x3_ep_f32 (csrc/conv3x3.hip), irm_conv3x3_f16x3_ep_f32 (csrc/conv3x3_f16.hip) and irm_conv3x3_thin_f32
(csrc/conv3x3_thin.hip) pick one of 24: CONV_VARIANTS, expected_conv_variant(); passes_per_group() restates how the
output-channel passes are dealt to the workgroup groups.  CONV_CASES places cases on each instantiation's edges (several
passes in one workgroup, groups with unequal pass counts, a ragged last pass, a last tile with Co % 16 != 0, a half-full
last input stage, partial row and column tiles, channel slices of larger buffers, the scalar and the 16-byte store path of
the generic kernel, every epilogue); CASE_STRUCTURES says which pass structures they run on each variant.  The launch
planner shrinks ct on images this small, so every case passes ct and ygroups explicitly (ops.plan_conv3x3 keeps explicit
values)."""
from irm_amd import ops

LN_NONE, LN_WB, LN_BF = 0, 1, 2
CTS = (3, 4, 6, 8, 9)                   # the ct switches of gemm_entry (gemm_pw.hip:656-662, 669-675, 678-684)
EXACT_CTS = (1, 2, 3, 4, 6)             # the two ct switches of irm_conv3x3_ep_f32 (conv3x3.hip)
SPLIT_CTS = (1, 2, 3, 4, 8, 12)         # output tiles per pass: the ct switch of irm_conv3x3_f16x3_ep_f32


# --------------------------------------------------------------------------- 1x1 GEMM: the variant table and its dispatch mirror
def gemm_ring(pt, ct, ns, ln, res, f16):
    return f"gemm_ring_kernel<{pt}, {ct}, {ns}, {ln}, {'true' if res else 'false'}, {'true' if f16 else 'false'}>"


def gemm_generic(ct, vec):
    return f"gemm_pw_kernel<2, {ct}, {'true' if vec else 'false'}>"


def xres(kt, ct):
    # xres_launch<KT, CT, NS = 3, NPT = 16, WP = 2>, KT 12: <12, CT, 3, 8, 2> (gemm_xres.hip:229-236, 248-253);
    # the kernel's own template order is <KT, CT, NS, WP, NPT>
    return f"gemm_xres_kernel<{kt}, {ct}, 3, 2, {8 if kt == 12 else 16}>"


def ring_ns(ct, k, f16):
    """Ring depth of a residual launch (PT 2): 3 for ct <= 6 and K <= 512 (the split kernel not at ct 4), else 4
    (launch_ring, gemm_pw.hip:560-577)."""
    return 3 if ct <= 6 and k <= 512 and not (f16 and ct == 4) else 4


def res_depths(ct, f16):
    return (3, 4) if ct <= 6 and not (f16 and ct == 4) else (4,)


VARIANTS = sorted(
    # exact f32 ring, residual: PT 2, no LN (launch_ring_any, gemm_pw.hip:584-587)
    [gemm_ring(2, ct, ns, LN_NONE, True, False) for ct in CTS for ns in res_depths(ct, False)]
    # exact f32 ring, no residual: PT 4 (3-deep ring) or PT 2 (4-deep), any LN (gemm_pw.hip:588-595)
    + [gemm_ring(pt, ct, 3 if pt == 4 else 4, ln, False, False) for pt in (2, 4) for ct in CTS for ln in (0, 1, 2)]
    # split ring, residual: PT 2, no LN (launch_ring_split, gemm_pw.hip:601-604)
    + [gemm_ring(2, ct, ns, LN_NONE, True, True) for ct in CTS for ns in res_depths(ct, True)]
    # split ring, no residual: PT 4 (gemm_pw.hip:605-607)
    + [gemm_ring(4, ct, 3, ln, False, True) for ct in CTS for ln in (0, 1, 2)]
    # generic streaming kernel (gemm_pw.hip:678-685 -> launch_gemm 610-617)
    + [gemm_generic(ct, vec) for ct in CTS for vec in (False, True)]
    # input-resident split kernel (gemm_xres.hip:246-253)
    + [xres(kt, ct) for kt in (2, 4, 6, 12) for ct in (8, 9)])
assert len(VARIANTS) == len(set(VARIANTS)) == 78


def expected_variant(*, split, M, K, N, B, ct, ygroups, ln, res, stats_out, w_bs, vec):
    """The instantiation gemm_entry launches (None = IRM_EINVAL).
    Mirrors gemm_pw.hip:626-686 and gemm_xres.hip:246-257."""
    mt = (M + 15) // 16
    if stats_out and mt > ct:                                       # gemm_pw.hip:644
        return None
    nchunks = -(-mt // ct)
    yg = min(max(ygroups, 1), nchunks)                              # gemm_pw.hip:645-647
    if split:
        if not vec or N < 4 or (res and ln):                        # gemm_pw.hip:651
            return None
        if K <= 192 and ln and not stats_out and not res and not w_bs:    # gemm_pw.hip:652
            st, kt_ct = (K + 15) // 16, 9 if mt % 9 == 0 else 8    # gemm_xres.hip:246
            if st in (2, 4, 6) or (st == 12 and M >= 512):          # gemm_xres.hip:247-256
                return xres(st, kt_ct)
        if ct not in CTS:
            return None
        if res:                                                     # gemm_pw.hip:601-604
            return gemm_ring(2, ct, ring_ns(ct, K, True), LN_NONE, True, True)
        return gemm_ring(4, ct, 3, ln, False, True)                 # gemm_pw.hip:605-607
    if ct not in CTS:
        return None
    if vec and N >= 4 and not (res and ln):                         # gemm_pw.hip:665
        if res:
            return gemm_ring(2, ct, ring_ns(ct, K, False), LN_NONE, True, False)
        pt = 4 if B * -(-N // 256) * yg >= 512 else 2               # gemm_pw.hip:668
        return gemm_ring(pt, ct, 3 if pt == 4 else 4, ln, False, False)
    return gemm_generic(ct, vec)                                    # gemm_pw.hip:678-685


# --------------------------------------------------------------------------- 3x3 conv: the variant table and its dispatch mirror
def conv_ring(ct):
    return f"conv3x3_ring_kernel<{ct}, 3>"              # launch_conv_ring (conv3x3.hip): NS = 3


def conv_generic(ct):
    return f"conv3x3_kernel<{ct}>"


def split(ct):
    """ct 1 ... 4: one weight chunk of ct tiles; 8 / 12: 2 / 3 chunks of 4 (the ct switch of irm_conv3x3_f16x3_ep_f32)."""
    return f"conv3x3_f16x3_kernel<{min(ct, 4)}, {max(1, ct // 4)}>"


def thin_in(ci):
    return f"conv3x3_thin_in_kernel<{ci}, 2>"


def thin_out(co):
    return f"conv3x3_thin_out_kernel<{co}, 4>"


CONV_VARIANTS = sorted([conv_ring(ct) for ct in EXACT_CTS] + [conv_generic(ct) for ct in EXACT_CTS]
                       + [split(ct) for ct in SPLIT_CTS]
                       + [thin_in(c) for c in (1, 2, 3, 4)] + [thin_out(c) for c in (1, 2, 3, 4)])
assert len(CONV_VARIANTS) == len(set(CONV_VARIANTS)) == 24


def expected_conv_variant(kind, ci, co, W, ct, x_bs, y_bs, r_bs, x_al, y_al, r_al, wp_al):
    """(instantiation, vec) the entry point of `kind` ("exact", "split", "thin") launches, None = IRM_EINVAL.  *_bs:
    batch strides in floats (0 without a residual), *_al: the pointer is 16-byte aligned (a null residual is).  vec is
    ConvArgs.vec, the 16-byte store path of the generic kernel; the split and the thin kernels always store 16 bytes."""
    all_vec = W % 4 == 0 and x_bs % 4 == 0 and y_bs % 4 == 0 and r_bs % 4 == 0 and x_al and y_al and r_al
    if kind == "exact":                                             # irm_conv3x3_ep_f32 (conv3x3.hip)
        if ct not in EXACT_CTS:
            return None
        vec = W % 4 == 0 and y_bs % 4 == 0 and r_bs % 4 == 0 and y_al and r_al      # a.vec
        fast = vec and x_bs % 4 == 0 and x_al and wp_al                             # fast
        return (conv_ring(ct) if fast else conv_generic(ct)), vec
    if kind == "split":                                             # irm_conv3x3_f16x3_ep_f32: alignment, ct switch
        if not (all_vec and wp_al) or ct not in SPLIT_CTS:
            return None
        return split(ct), True
    if kind == "thin":                                              # irm_conv3x3_thin_f32: checks, Co / Ci dispatch
        if not all_vec or (co > 4 and ci > 4):
            return None
        return (thin_out(co) if co <= 4 and ci > 4 else thin_in(ci)), True
    raise ValueError(kind)


def passes_per_group(mtiles, ct, ygroups):
    """Output-channel passes each workgroup group runs: ygroups is clamped to [1, nchunks] (irm_conv_common,
    conv_epilogue.h) and group y takes passes y, y + ygroups, ... (my_chunks in conv3x3_ring_kernel)."""
    nchunks = -(-mtiles // ct)
    yg = min(max(ygroups, 1), nchunks)
    return [(nchunks - y + yg - 1) // yg for y in range(yg)]


def pass_structure(passes):
    """"single": no workgroup runs a second pass; else "even" or "uneven" pass counts over the groups."""
    return "single" if max(passes) == 1 else "even" if min(passes) == max(passes) else "uneven"


# --------------------------------------------------------------------------- 3x3 conv: cases
def conv_case(kind, path, name, co, ci, H, W, *, B=2, ct=None, yg=None, bias=False, relu1=False, res_mode=0, relu2=False,
              store_mode=0, shuffle=2, leaky=None, x_off=0, y_off=0, r_off=0):
    """One launch.  path: "ring" / "scalar" / "vec" (exact), "split", "thin"; *_off: floats the buffer starts past a
    16-byte boundary."""
    return dict(kind=kind, path=path, name=name, co=co, ci=ci, H=H, W=W, B=B, ct=ct, yg=yg, bias=bias, relu1=relu1,
                res_mode=res_mode, relu2=relu2, store_mode=store_mode, shuffle=shuffle, leaky=leaky, x_off=x_off,
                y_off=y_off, r_off=r_off)


def _exact_cases(ct, path):
    """Cases A - D of one exact CT on one path: the ring (all aligned, W = 36), the generic kernel with scalar stores
    (W = 35; once W = 36 with every buffer one float past alignment) or with 16-byte stores (W = 36, only x one float
    past alignment).  The PixelUnshuffle case takes W = 40 instead of 36 (its output planes, 5 x 18 floats at W = 36,
    would put the output slice off 16-byte alignment and the launch on the scalar path) and W = 38 on the scalar path."""
    W = 35 if path == "scalar" else 36
    off = dict(x_off=1) if path == "vec" else {}
    kw = dict(ct=ct, **off)
    cases = [
        conv_case("exact", path, "A uneven-groups ragged-last-pass relu res1 relu2", 16 * (2 * ct + 1) - 1, 20, 9, W, yg=2,
                  bias=True, relu1=True, res_mode=1, relu2=True, **kw),
        conv_case("exact", path, "B one-pass m%16=1 res2", 16 * (ct - 1) + 1, 5, 5, W, yg=1, res_mode=2, **kw),
        conv_case("exact", path, "C three-passes one-stage shuffle2", 48 * ct, 3, 5, W, yg=1, store_mode=2, shuffle=2, **kw),
        conv_case("exact", path, "C three-passes one-stage shuffle4", 48 * ct, 3, 5, W, yg=1, store_mode=2, shuffle=4, **kw),
        conv_case("exact", path, "D two-passes ragged unshuffle", 16 * ct + 8, 12, 10, 38 if path == "scalar" else 40, yg=1,
                  store_mode=1, **kw),
    ]
    if path == "scalar":
        cases.append(conv_case("exact", path, "A all-buffers-offset", 16 * (2 * ct + 1) - 1, 20, 9, 36, yg=2, bias=True,
                               relu1=True, res_mode=1, relu2=True, ct=ct, x_off=1, y_off=1, r_off=1))
    if ct == 3:
        cases.append(conv_case("exact", path, "B ygroups-100-clamped", 16 * (ct - 1) + 1, 5, 5, W, yg=100, res_mode=2, **kw))
    return cases


def _exact_epilogue_cases(path):
    """Once per path: the tanh + clamp residual (res_mode 3) and LeakyReLU."""
    W = 35 if path == "scalar" else 36
    off = dict(x_off=1) if path == "vec" else {}
    return [
        conv_case("exact", path, "E tanh-clamp two-groups", 40, 9, 9, W, ct=2, yg=2, bias=True, res_mode=3, **off),
        conv_case("exact", path, "F leaky two-passes", 50, 9, 9, W, ct=3, yg=1, bias=True, leaky=0.1, **off),
    ]


def _split_cases(ct):
    """A, C, D with CT = the output tiles per pass, W = 36 and aligned slices (the kernel accepts nothing else), and B
    for the single-pass launch production issues most."""
    return [
        conv_case("split", "split", "A uneven-groups ragged-last-pass relu res1 relu2", 16 * (2 * ct + 1) - 1, 40, 9, 36,
                  ct=ct, yg=2, bias=True, relu1=True, res_mode=1, relu2=True),
        conv_case("split", "split", "B one-pass m%16=1 res2", 16 * (ct - 1) + 1, 5, 5, 36, ct=ct, yg=1, res_mode=2),
        conv_case("split", "split", "C three-passes one-stage shuffle2", 48 * ct, 3, 5, 36, ct=ct, yg=1, store_mode=2),
        conv_case("split", "split", "C three-passes one-stage shuffle4", 48 * ct, 3, 5, 36, ct=ct, yg=1, store_mode=2,
                  shuffle=4),
        conv_case("split", "split", "D two-passes ragged unshuffle", 16 * ct + 8, 70, 10, 40, ct=ct, yg=1, store_mode=1),
    ]


def _thin_cases():
    cases = [
        conv_case("thin", "thin", "ragged co group 13+13+13+11", 50, 3, 9, 12, B=1, bias=True, relu1=True),
        conv_case("thin", "thin", "ragged co group 10+9 B3", 19, 2, 5, 8, B=3, res_mode=1, relu2=True),
        conv_case("thin", "thin", "gray first layer odd H", 17, 1, 7, 8, bias=True, relu1=True),
        conv_case("thin", "thin", "ci4 ragged co group 9+9+9+6", 33, 4, 9, 12, B=1, bias=True, res_mode=2),
    ]
    for co in (1, 2, 3, 4):     # H = 6: the second 4-row strip holds 2 rows; Ci = 9: the four waves sum 3, 2, 2, 2 channels
        cases.append(conv_case("thin", "thin", f"co{co} partial strip", co, 9, 6, 12, bias=co % 2 == 1,
                               res_mode=(0, 1, 2, 3)[co - 1], relu1=co == 2, relu2=co == 4))
    return cases


CONV_CASES = []
for _ct in EXACT_CTS:
    for _path in ("ring", "scalar", "vec"):
        CONV_CASES += _exact_cases(_ct, _path)
for _path in ("ring", "scalar", "vec"):
    CONV_CASES += _exact_epilogue_cases(_path)
for _ct in SPLIT_CTS:
    CONV_CASES += _split_cases(_ct)
CONV_CASES += _thin_cases()


# --------------------------------------------------------------------------- 3x3 conv: layouts
def out_shape(c):
    """(channels, H, W) of the output tensor."""
    co, H, W, r = c["co"], c["H"], c["W"], c["shuffle"]
    if c["store_mode"] == 1:
        return co * 4, H // 2, W // 2
    if c["store_mode"] == 2:
        return co // (r * r), H * r, W * r
    return co, H, W


def layout(c):
    """Batch strides (floats) and 16-byte alignment of x, y, res of a case: x is channels [2, 2 + Ci) of a Ci + 3
    channel buffer, y channels [1, 1 + C_out) of C_out + 2, res channels [1, 1 + Co) of Co + 3 (allocations are 16-byte
    aligned; *_off floats are skipped in front)."""
    N = c["H"] * c["W"]
    oc, oh, ow = out_shape(c)
    lay = dict(x_bs=(c["ci"] + 3) * N, x_al=(c["x_off"] + 2 * N) % 4 == 0,
               y_bs=(oc + 2) * oh * ow, y_al=(c["y_off"] + oh * ow) % 4 == 0, r_bs=0, r_al=True)
    if c["res_mode"]:
        lay.update(r_bs=(c["co"] + 3) * N, r_al=(c["r_off"] + N) % 4 == 0)
    return lay


def case_plan(c):
    """(ct, ygroups) the launch gets from ops.conv3x3 (the thin kernel has no plan)."""
    if c["kind"] == "thin":
        return None, None
    return ops.plan_conv3x3(c["co"], c["H"], c["W"], c["B"], split=c["kind"] == "split", ct=c["ct"], ygroups=c["yg"])


def case_variant(c):
    ct, _ = case_plan(c)
    return expected_conv_variant(c["kind"], c["ci"], c["co"], c["W"], ct, wp_al=True, **layout(c))


def case_passes(c):
    ct, yg = case_plan(c)
    return passes_per_group((c["co"] + 15) // 16, ct, yg)


def _variant_name(c):
    v = case_variant(c)
    if v is None:
        return "rejected"
    return v[0] + (" vec" if c["path"] == "vec" else " scalar" if c["path"] == "scalar" else "")


CONV_CASE_IDS = [f"{_variant_name(c)} | {c['name']}".replace(" ", "_") for c in CONV_CASES]
assert len(set(CONV_CASE_IDS)) == len(CONV_CASE_IDS)

#: variant -> the pass structures ("single" / "even" / "uneven") its cases run; tests/test_planner_cpu.py and
#: tests/test_gpu_launch_replay.py hold the planner's and production's launches against it
CASE_STRUCTURES = {}
for _c in CONV_CASES:
    _v = case_variant(_c)
    if _v is not None:
        CASE_STRUCTURES.setdefault(_v[0], set()).add("single" if _c["kind"] == "thin" else pass_structure(case_passes(_c)))
