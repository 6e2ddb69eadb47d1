"""The update-block descriptor sweep: the case table and a float64 composition of the four refinement loops.  CPU-importable.

The library accepts hidden_dim = any multiple of 32, context_dim = any multiple of 8, cor_planes = levels * (2r + 1) [* groups],
1 or 2 flow channels, both GRUs and rates 4 / 8; each case below is one point of that space chosen for the launch or the
instantiation it reaches (`why`).  tests/test_desc_sweep_cpu.py pins this module against the oracle and measures the fp32 oracle's
own drift from float64; tests/test_gpu_desc_sweep.py runs every case in the three arithmetics against the float64 composition.

The composition is built from the oracle's dtype-agnostic pieces (R.corr1d_build, R.linear_sampler, R.update_block,
R.convex_upsample, R.igev_pyramids, R.raft_group_corr_build, cre_ref.agcl_corr_iter).  The oracle's three lookups end in
`.float()`, so they are restated here without the cast (`raft_lookup`, `igev_lookup`, `group_lookup`); in float32 they return the
oracle's bits."""
import functools
import zlib

import torch

from nndepth_amd import weightgen
from oracle import cre_ref as CR
from oracle import torch_ref as R

B, H, W = 2, 13, 22  # ragged on both axes of the 4x8 pixel tile, two batch items (the map of the split tests)
ITERS = 3
ARITHS = ("fp32", "bf16x3", "fp16x2")
RUNS = ("zero", "wide")  # initial disparity / flow: zero | (rand - 0.5) * 2 * W: every lookup level samples beyond both borders


def _case(name, hid, ctx, loop, levels, radius, groups, rate, gru, fc, C, up, why):
    """up: "fused" = mask.2 inside the mask + upsample kernel (2 * hid in {128, 256}), "unfused" = mask.2 conv + convex upsample."""
    return dict(name=name, hid=hid, ctx=ctx, loop=loop, levels=levels, radius=radius, groups=groups, rate=rate,
                gru={"sep": "sep_conv", "conv": "conv_gru"}[gru], fc=fc, C=C, up=up, why=why)


CASES = [
    _case("h64_r8", 64, 64, "raft", 4, 4, 0, 8, "sep", 1, 256, "fused", "launch_mu<8,128>, folded flow head at hid 64, merged flow-branch+lookup"),
    _case("h64_r8_f2", 64, 64, "cre", 0, 0, 0, 8, "sep", 2, 64, "fused", "launch_mu<8,128> with 2 flow channels"),
    _case("h128_f2_c8", 128, 8, "cre", 0, 0, 0, 8, "sep", 2, 128, "fused", "smallest context with 2 flow channels"),
    _case("h96", 96, 40, "raft", 3, 4, 0, 8, "sep", 1, 128, "unfused", "27 planes (odd), unfused upsample, GRU Cin 232: exact fallback inside split blobs"),
    _case("h32", 32, 8, "raft", 2, 3, 0, 8, "sep", 1, 64, "unfused", "smallest descriptor, 14 planes, encoder.conv Cout 31"),
    _case("h160", 160, 72, "raft", 4, 5, 0, 4, "conv", 1, 256, "unfused", "44 planes, hid > 128, mask Cin 320"),
    _case("h64_l1", 64, 128, "raft", 1, 2, 0, 4, "sep", 1, 256, "fused", "5 planes, launch_mu<4,128>"),
    _case("h128_21", 128, 64, "raft", 3, 3, 0, 8, "sep", 1, 48, "fused", "default hidden, 21 planes, C = 48"),
    _case("h64_cg", 64, 24, "raft", 4, 4, 0, 8, "conv", 1, 24, "fused", "conv_gru with launch_mu<8,128>, C < 32 build"),
    _case("h128_r4", 128, 128, "raft", 4, 3, 0, 4, "sep", 1, 256, "fused", "28 planes, launch_mu<4,256> with the sep GRU"),
    _case("ig_l2", 64, 64, "igev", 2, 4, 8, 4, "sep", 1, 0, "fused", "interleaved kernel at 2 levels (288 planes)"),
    _case("ig_g4", 64, 64, "igev", 4, 4, 4, 4, "sep", 1, 0, "fused", "interleaved kernel unsupported, 288 planes: stand-alone lookup + split convc1"),
    _case("ig_r3", 128, 64, "igev", 3, 3, 8, 4, "sep", 1, 0, "fused", "336 planes, radius != 4"),
    _case("ig_g3", 64, 40, "igev", 3, 4, 3, 4, "sep", 1, 0, "fused", "162 planes (no multiple of 16): lookup_convc1_kernel<true>, partial last chunk"),
    _case("grp_g8", 64, 64, "group", 1, 3, 8, 4, "conv", 1, 64, "fused", "group lookup with G != 4, r != 4"),
]
# hidden sizes above the table's: either refused when the engine is built or held to the same bars (test_gpu_desc_sweep.py)
LARGE_HIDDEN = [
    _case("h192", 192, 64, "raft", 4, 4, 0, 8, "sep", 1, 64, "unfused", "hidden 192: flow_head.conv2 stages 57 KB of LDS"),
    _case("h256", 256, 64, "raft", 4, 4, 0, 8, "sep", 1, 64, "unfused", "hidden 256: flow_head.conv2 would need 75 KB of LDS"),
]
BY_NAME = {c["name"]: c for c in CASES + LARGE_HIDDEN}


def cor_planes(c) -> int:
    if c["loop"] == "cre":
        return 36
    taps = c["levels"] * (2 * c["radius"] + 1)
    return taps * {"raft": 1, "igev": 2 * c["groups"], "group": c["groups"]}[c["loop"]]


def gru_cin(c) -> int:
    return 2 * c["hid"] + c["ctx"]


def block_kwargs(c) -> dict:
    """BasicUpdateBlock's constructor arguments (without `arithmetic`)."""
    return dict(hidden_dim=c["hid"], cor_planes=cor_planes(c), context_dim=c["ctx"], gru=c["gru"], flow_channel=c["fc"],
                spatial_scale=c["rate"])


PREFIX = "sweep"


@functools.lru_cache(maxsize=None)
def _state_dict(name):
    c = BY_NAME[name]
    return weightgen.fill_state_dict(R.update_block_spec(f"{PREFIX}.{name}", c["hid"], cor_planes(c), c["ctx"], c["fc"], c["rate"], gru=c["gru"]))


def state_dict(c, dtype=torch.float32, strip=False):
    """Generated weights of the case's block; strip: keys as BasicUpdateBlock.load_state_dict takes them."""
    cut = len(f"{PREFIX}.{c['name']}.") if strip else 0
    return {k[cut:]: v.to(dtype) for k, v in _state_dict(c["name"]).items()}


def prefix(c) -> str:
    return f"{PREFIX}.{c['name']}"


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x = dict(net=torch.tanh(torch.randn(B, c["hid"], H, W, generator=g)), inp=torch.relu(torch.randn(B, c["ctx"], H, W, generator=g)))
    if c["loop"] == "igev":  # the two group volumes themselves, rows (b, g, h, w1) like R.igev_pyramids
        x["feat"] = torch.randn(B, c["groups"], H, W, W, generator=g)
        x["geo"] = torch.randn(B, c["groups"], W, H, W, generator=g)  # (B, G, W2, H, W1): as the regulariser returns it
    else:
        x["f1"], x["f2"] = torch.randn(B, c["C"], H, W, generator=g), torch.randn(B, c["C"], H, W, generator=g)
    x["wide"] = (torch.rand(B, c["fc"], H, W, generator=g) - 0.5) * 2 * W
    return x


def inputs(c, dtype=torch.float32) -> dict:
    """Seeded float32 inputs of the case (never modified), cast to dtype: net, inp, the feature maps or the IGEV volumes, and
    `wide`, the large initial disparity / flow."""
    return {k: v.to(dtype) for k, v in _inputs(c["name"]).items()}


def init_of(c, run, x):
    return None if run == "zero" else x["wide"]


# ---------------------------------------------------------------- the oracle's lookups without the final .float()
def raft_lookup(pyr, coords, num_levels, radius):
    """R.corr1d_lookup."""
    Bn, _, Hn, Wn = coords.shape
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=coords.dtype).view(1, -1)
    outs = []
    for i in range(num_levels):
        row = pyr[i].reshape(Bn * Hn * Wn, -1)
        x = dx + coords.reshape(Bn * Hn * Wn, 1) / 2 ** i
        outs.append(R.linear_sampler(row, x).view(Bn, Hn, Wn, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def igev_lookup(fp, gp, coords, num_groups, num_levels, radius):
    """R.igev_lookup: channel = level * 2GT + volume * GT + group * T + tap."""
    Bn, _, Hn, Wn = coords.shape
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=coords.dtype).reshape(1, -1)
    outs = []
    for i in range(num_levels):
        c = coords.permute(0, 2, 3, 1).unsqueeze(1).repeat(1, num_groups, 1, 1, 1)
        x = c.reshape(Bn * num_groups * Hn * Wn, 1) / 2 ** i + dx
        for pyr in (fp, gp):
            s = R.linear_sampler(pyr[i].reshape(Bn * num_groups * Hn * Wn, -1), x)
            outs.append(s.reshape(Bn, num_groups, Hn, Wn, -1).permute(0, 2, 3, 1, 4).reshape(Bn, Hn, Wn, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def group_lookup(pyr, coords, num_groups, num_levels, radius):
    """R.raft_group_corr_lookup (the view that does not move the group axis included)."""
    Bn, _, Hn, Wn = coords.shape
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=coords.dtype).view(1, -1)
    outs = []
    for i in range(num_levels):
        row = pyr[i].reshape(Bn * num_groups * Hn * Wn, -1)
        c = coords.permute(0, 2, 3, 1).unsqueeze(1).repeat(1, num_groups, 1, 1, 1)
        x = dx + c.reshape(Bn * num_groups * Hn * Wn, 1) / 2 ** i
        outs.append(R.linear_sampler(row, x).view(Bn, Hn, Wn, -1))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def build_pyramids(c, x):
    """The case's correlation pyramid(s) in the dtype of x: raft / group: one list; igev: (feature, geometry)."""
    if c["loop"] == "raft":
        return R.corr1d_build(x["f1"], x["f2"], c["levels"])
    if c["loop"] == "group":
        return R.raft_group_corr_build(x["f1"], x["f2"], c["groups"], c["levels"])
    if c["loop"] == "igev":
        return R.igev_pyramids(x["feat"], x["geo"], c["levels"])
    return None


def lookup(c, pyr, x, state, it):
    """The sampled correlation features the update block of iteration `it` receives; state: the coordinate (the flow for cre)."""
    if c["loop"] == "raft":
        return raft_lookup(pyr, state, c["levels"], c["radius"])
    if c["loop"] == "group":
        return group_lookup(pyr, state, c["groups"], c["levels"], c["radius"])
    if c["loop"] == "igev":
        return igev_lookup(pyr[0], pyr[1], state, c["groups"], c["levels"], c["radius"])
    return CR.agcl_corr_iter(x["f1"], x["f2"], state, it % 2 == 1)


def oracle_lookup(c, pyr, x, state, it):
    """The same through the oracle's own functions (float32 out)."""
    if c["loop"] == "raft":
        return R.corr1d_lookup(pyr, state, c["levels"], c["radius"])
    if c["loop"] == "group":
        return R.raft_group_corr_lookup(pyr, state, c["groups"], c["levels"], c["radius"])
    if c["loop"] == "igev":
        return R.igev_lookup(pyr[0], pyr[1], state, c["groups"], c["levels"], c["radius"])
    return CR.agcl_corr_iter(x["f1"], x["f2"], state, it % 2 == 1)


# ---------------------------------------------------------------- the loops
def compose(c, dtype, run, iters=ITERS) -> dict:
    """The case's refinement loop in `dtype` from `run`'s initial state -> ups (one map per iteration), low (the final
    low-resolution state as the engine returns it: disparity; absolute coordinate for igev; flow for cre), net, and states (what
    each iteration's lookup sampled at).
      raft / group: R.raft_stereo_forward's / R.coarse2fine_refine's loop;  igev: R.igev_refine;  cre: the last stage of
      cre_ref.cre_stereo_forward (iter mode: 3x3 window on odd iterations, 1x9 on even ones)."""
    x = inputs(c, dtype)
    sd, p = state_dict(c, dtype), prefix(c)
    pyr = build_pyramids(c, x)
    net, inp = x["net"], x["inp"]
    init = init_of(c, run, x)
    org = torch.arange(W, dtype=dtype)[None, None, None, :].repeat(B, 1, H, 1)
    if c["loop"] == "cre":
        state = torch.zeros(B, 2, H, W, dtype=dtype) if init is None else init.clone()
    else:
        state = org.clone() if init is None else org + init
    ups, states = [], []
    for it in range(iters):
        states.append(state)
        samp = lookup(c, pyr, x, state, it)
        flow = state if c["loop"] in ("cre", "igev") else state - org  # igev: the block and the upsample take the coordinate itself
        net, mask, delta = R.update_block(sd, p, net, inp, samp, flow, gru=c["gru"])
        state = state + delta
        ups.append(R.convex_upsample(state if c["loop"] in ("cre", "igev") else state - org, mask, c["rate"]))
    low = state if c["loop"] in ("cre", "igev") else state - org
    return dict(ups=ups, low=low, net=net, states=states)


@functools.lru_cache(maxsize=None)
def _reference(name, run):
    with torch.no_grad():
        return compose(BY_NAME[name], torch.float64, run)


def reference(c, run) -> dict:
    """The float64 composition, computed once per (case, run) and shared; do not modify."""
    return _reference(c["name"], run)


@functools.lru_cache(maxsize=None)
def _block_once(name):
    """One application of the block at a moderate flow (|flow| < 4, non-zero on every pixel): the features from the float64 lookup
    at that flow, every input rounded to float32 (what the kernel receives), and the float64 outputs on those inputs."""
    c = BY_NAME[name]
    x = inputs(c, torch.float64)
    flow = x["wide"] * (4.0 / W)
    org = torch.arange(W, dtype=torch.float64)[None, None, None, :].repeat(B, 1, H, 1)
    state = flow if c["loop"] == "cre" else org + flow
    blk_flow = state if c["loop"] in ("cre", "igev") else flow
    with torch.no_grad():
        corr = lookup(c, build_pyramids(c, x), x, state, 1)
        ins = [t.float() for t in (x["net"], x["inp"], corr, blk_flow)]
        outs = R.update_block(state_dict(c, torch.float64), prefix(c), *(t.double() for t in ins), gru=c["gru"])
    return ins, outs


def block_once(c):
    """-> ([net, inp, corr, flow] float32, (net, mask, delta) float64), computed once per case; do not modify."""
    return _block_once(c["name"])


# ---------------------------------------------------------------- the report both test modules write
REPORT_HEADER = ("Update-block descriptor sweep (tests/desc_sweep_cases.py): max-abs error against the float64 composition of each loop,\n"
                 f"{B}x{H}x{W} map, {ITERS} iterations.  run zero: from zero; run wide: from (rand - 0.5) * 2 * W.\n")
CPU_MARK = "== fp32 oracle vs float64 (tests/test_desc_sweep_cpu.py)\n"
GPU_MARK = "== HIP vs float64 on MI355X (tests/test_gpu_desc_sweep.py)\n"


def report_split(text: str):
    """-> (cpu block, gpu block) of an existing report ('' where missing)."""
    cpu = gpu = ""
    if CPU_MARK in text:
        cpu = text.split(CPU_MARK, 1)[1].split(GPU_MARK, 1)[0]
    if GPU_MARK in text:
        gpu = text.split(GPU_MARK, 1)[1]
    return cpu, gpu


def report_join(cpu: str, gpu: str) -> str:
    return REPORT_HEADER + CPU_MARK + cpu + (GPU_MARK + gpu if gpu else "")


def oracle_drift(cpu_block: str) -> dict:
    """{(case, run): drift of the fp32 oracle on the upsampled maps} from the report's CPU block."""
    out = {}
    for line in cpu_block.splitlines():
        f = line.split()
        if len(f) >= 4 and f[0] in BY_NAME and f[1] in RUNS:
            out[(f[0], f[1])] = float(f[2])
    return out
