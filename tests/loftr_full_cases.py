"""Cases and float64 contract of the LoFTR full (softmax) attention (csrc/attention.hip, nnd_loftr_full_layer_forward).

Shared by scripts/make_golden_loftr_full.py (which writes tests/golden/loftr_full.npz), tests/test_loftr_full_cpu.py and
tests/test_gpu_loftr_full.py.  Every input is a pure function of the case's name through nndepth_amd.weightgen, so the fixture
stores no input array; the layer weights are weightgen.fill_state_dict(oracle.cre_ref.cre_stereo_spec()).

Names:
  att/<N>x<nhead>x<L>x<S>/g<scale>      Gaussian q, k, v (N, nhead*32, L|S), all three times scale
  att/<N>x<nhead>x<L>x<S>/qv16          Gaussian, q and v times 16, k as it is: logits to 64 .. 86 (see REFUSED)
  att/<N>x<nhead>x<L>x<S>/spike_last    Gaussian, every query's maximum on key S-1 (last KV tile), gap ~350: the online softmax's
  att/<N>x<nhead>x<L>x<S>/spike_first   rescale factor ends at exactly 0; ... on key 0 (first tile): the factor stays 1
  layer/<N>x<H>x<W>/<cross|self>/g<scale>   Gaussian maps (N, 256, H, W) times scale; self: source = x
"""
import functools
import json
import math
import os

import numpy as np
import torch

from nndepth_amd import weightgen

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D_MODEL, NHEAD, HEAD = 256, 8, 32
SCALES = (1, 4, 16)
GATHER_SHAPES = ((1, 8, 1, 1), (1, 2, 33, 65), (2, 8, 40, 97), (1, 8, 97, 40), (2, 8, 135, 135))  # N, nhead, L, S
ATT_SHAPES = GATHER_SHAPES[1:]
SPIKE_SHAPE = (2, 8, 135, 135)
LAYER_SHAPES = ((1, 1, 1), (2, 5, 8), (1, 3, 11), (1, 7, 9), (2, 9, 15), (1, 17, 30))  # N, H, W
STYLES = ("cross", "self")
CAP = 7.5e-6  # the fixture refuses a case whose reference fp32 result is further than CAP * max(1, fmax) from the contract

# Refused by the fixture's cap, at every shape: with q, k and v all times 16 the logits reach 1000 .. 1400, a logit carries an fp32
# rounding error of ~1e-4, and the softmax of Gaussian scores has near ties that pass it on: the reference's own fp32 result is
# 1.5e-5 .. 3.6e-5 * fmax from the contract (tests/golden/REPORT_loftr_full.txt).  The cases stay listed and are in no fixture and
# no test; what they were for (a kernel that forgets the max subtraction overflows) is covered by the spike cases (logit ~390),
# the layer cases at x16 (logits to 1100, saturated softmax) and the exact gather (2896).  The qv16 cases keep a x16 case per shape
# that is well conditioned.
REFUSED = tuple(f"att/{n}x{h}x{l}x{s}/g16" for n, h, l, s in ATT_SHAPES)
ATT_CASES = tuple(c for c in (f"att/{n}x{h}x{l}x{s}/g{g}" for n, h, l, s in ATT_SHAPES for g in SCALES) if c not in REFUSED) + tuple(
    f"att/{n}x{h}x{l}x{s}/qv16" for n, h, l, s in ATT_SHAPES) + tuple(
    "att/%dx%dx%dx%d/%s" % (SPIKE_SHAPE + (k,)) for k in ("spike_last", "spike_first"))
LAYER_CASES = tuple(f"layer/{n}x{h}x{w}/{st}/g{g}" for n, h, w in LAYER_SHAPES for st in STYLES for g in SCALES)
CASES = ATT_CASES + LAYER_CASES
# the two layer cases whose reference fp32 output the fixture stores: the two smallest shapes, one of each style
STORED = ("layer/1x1x1/cross/g1", "layer/1x3x11/self/g4")


def gaussian(tag: str, *shape) -> torch.Tensor:
    """Standard normal float32 values, a pure function of (tag, shape): Box-Muller in float64 on weightgen.uniform01."""
    n = int(np.prod(shape))
    u1 = weightgen.uniform01(tag + "/u1", n).astype(np.float64)
    u2 = weightgen.uniform01(tag + "/u2", n).astype(np.float64)
    z = np.sqrt(-2.0 * np.log1p(-u1)) * np.cos(2.0 * np.pi * u2)
    return torch.from_numpy(z.astype(np.float32).reshape(shape))


def _dims(name: str):
    return tuple(int(t) for t in name.split("/")[1].split("x"))


@functools.lru_cache(maxsize=None)
def make_case(name: str):
    """att/...: (q, k, v, nhead); layer/...: (prefix, x, source).  CPU float32 tensors, made once: do not modify."""
    parts = name.split("/")
    if parts[0] == "att":
        n, nhead, l, s = _dims(name)
        c = nhead * HEAD
        q, k, v = gaussian(name + "/q", n, c, l), gaussian(name + "/k", n, c, s), gaussian(name + "/v", n, c, s)
        if parts[2].startswith("spike"):
            key = s - 1 if parts[2] == "spike_last" else 0
            q = q + 8.0
            k[:, :, key] = 8.0  # score (8 sum_d q + 2048) / sqrt(32) ~ 362 +- 8 against ~ 0 +- 8 elsewhere
        elif parts[2] == "qv16":
            q, v = q * 16.0, v * 16.0
        else:
            g = float(parts[2][1:])
            q, k, v = q * g, k * g, v * g
        return q, k, v, nhead
    n, h, w = _dims(name)
    g = float(parts[3][1:])
    x = gaussian(name + "/x", n, D_MODEL, h, w) * g
    source = x if parts[2] == "self" else gaussian(name + "/source", n, D_MODEL, h, w) * g
    return f"{parts[2]}_att_fn.layers.0.", x, source


@functools.lru_cache(maxsize=None)
def state_dict():
    from oracle import cre_ref
    return weightgen.fill_state_dict(cre_ref.cre_stereo_spec())


# ------------------------------------------------------------------------------------------------ float64 contract
def _f64(t) -> np.ndarray:
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float64)


def contract64_attention(q, k, v, nhead: int) -> np.ndarray:
    """out[n, 32h+d, l] = sum_s softmax_s((sum_d q[n,32h+d,l] k[n,32h+d,s]) / sqrt(32)) v[n,32h+d,s], float64.
    q (N, nhead*32, L), k and v (N, nhead*32, S) -> (N, nhead*32, L)."""
    q, k, v = _f64(q), _f64(k), _f64(v)
    n, c, l = q.shape
    s = k.shape[2]
    assert c == nhead * HEAD and k.shape == v.shape == (n, c, s)
    qh, kh, vh = q.reshape(n, nhead, HEAD, l), k.reshape(n, nhead, HEAD, s), v.reshape(n, nhead, HEAD, s)
    score = np.einsum("nhdl,nhds->nhls", qh, kh) / math.sqrt(HEAD)
    e = np.exp(score - score.max(axis=3, keepdims=True))
    p = e / e.sum(axis=3, keepdims=True)
    return np.einsum("nhls,nhds->nhdl", p, vh).reshape(n, c, l)


def _layernorm64(t: np.ndarray, gamma: np.ndarray, beta: np.ndarray) -> np.ndarray:
    """LayerNorm over the channel axis (axis 1) of (N, C, L), eps 1e-5, biased variance, with affine."""
    mu = t.mean(axis=1, keepdims=True)
    var = ((t - mu) ** 2).mean(axis=1, keepdims=True)
    return (t - mu) / np.sqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]


def contract64_layer(sd, prefix: str, x, source) -> np.ndarray:
    """The layer on (N, C, H, W) maps in float64: msg = attention(Wq x, Wk s, Wv s); m = LN1(Wm msg);
    m = LN2(W2 relu(W1 [x | m])); out = x + m."""
    w = {k: _f64(sd[prefix + k]) for k in ("q_proj.weight", "k_proj.weight", "v_proj.weight", "merge.weight", "mlp.0.weight",
                                           "mlp.2.weight", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")}
    x, source = _f64(x), _f64(source)
    shape = x.shape
    n, c = shape[:2]
    x, source = x.reshape(n, c, -1), source.reshape(n, c, -1)
    lin = lambda wt, t: np.einsum("oc,ncl->nol", wt, t)
    msg = contract64_attention(lin(w["q_proj.weight"], x), lin(w["k_proj.weight"], source), lin(w["v_proj.weight"], source), c // HEAD)
    m = _layernorm64(lin(w["merge.weight"], msg), w["norm1.weight"], w["norm1.bias"])
    hid = np.maximum(lin(w["mlp.0.weight"], np.concatenate([x, m], axis=1)), 0.0)
    m = _layernorm64(lin(w["mlp.2.weight"], hid), w["norm2.weight"], w["norm2.bias"])
    return (x + m).reshape(shape)


@functools.lru_cache(maxsize=None)
def contract(name: str) -> np.ndarray:
    """The float64 contract of a case, computed once and shared: read-only."""
    c = make_case(name)
    out = contract64_attention(*c) if name.startswith("att/") else contract64_layer(state_dict(), *c)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ fixture and bar
@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLD, "loftr_full.npz"))
    names = json.loads(str(z["names"]))
    fx = {n: {"d_ref": float(d), "fmax": float(f)} for n, d, f in zip(names, z["d_ref"], z["fmax"])}
    for n in STORED:
        fx[n]["ref_out"] = z["ref_out/" + n]
    return fx


def bar(name: str) -> float:
    """max(4 d_ref, 4 * 2^-23 * fmax): d_ref is the reference's own fp32 distance from the contract (fixture); 4 = 2 (a second,
    independent fp32 evaluation order, compared by the maximum over 1e4 .. 1e6 outputs) x 2 (the MFMA's k-ordered fmaf chain has
    no blocked summation, unlike the CPU library's dot products); the floor is four ulp of the largest output."""
    fx = fixture()[name]
    return max(4.0 * fx["d_ref"], 4.0 * 2.0 ** -23 * fx["fmax"])


# ------------------------------------------------------------------------------------------------ exact gather
def gather_case(n: int, nhead: int, l: int, s: int):
    """q, k, v, pi: k[:, :, j] in {+-1}^32 per head with the bits of j in its first 13 coordinates (distinct keys, any two differ
    in a coordinate); q[..., i] = 512 k[..., pi(i)], pi(i) = (7 i + 3) mod s; v Gaussian.  The winning score is 512 * 32 / sqrt(32)
    ~ 2896, every other at most 512 * 28 / sqrt(32) ~ 2534 .. 2715: softmax is exactly one-hot in fp32 and out[..., i] must be
    v[..., pi(i)] bit for bit."""
    j = np.arange(s)
    key = np.ones((HEAD, s), np.float32)
    for b in range(13):
        key[b] = np.where((j >> b) & 1, 1.0, -1.0)
    # the other 19 coordinates: signs that differ per head and key, from the generator
    rest = weightgen.uniform01(f"gather/{n}x{nhead}x{l}x{s}/signs", n * nhead * 19 * s).reshape(n, nhead, 19, s)
    k = np.empty((n, nhead, HEAD, s), np.float32)
    k[:, :, :13] = key[:13]
    k[:, :, 13:] = np.where(rest < 0.5, -1.0, 1.0)
    pi = (7 * np.arange(l) + 3) % s
    q = 512.0 * k[:, :, :, pi]
    v = gaussian(f"gather/{n}x{nhead}x{l}x{s}/v", n, nhead * HEAD, s)
    return (torch.from_numpy(q.reshape(n, nhead * HEAD, l)), torch.from_numpy(k.reshape(n, nhead * HEAD, s)), v, torch.from_numpy(pi))


def gather_margin(q, k, nhead: int, pi) -> float:
    """Smallest (winning score - best other score) over every query, float64, in units of the scaled logit."""
    q, k = _f64(q), _f64(k)
    n, c, l = q.shape
    s = k.shape[2]
    score = np.einsum("nhdl,nhds->nhls", q.reshape(n, nhead, HEAD, l), k.reshape(n, nhead, HEAD, s)) / math.sqrt(HEAD)
    pi = np.asarray(pi)
    win = np.take_along_axis(score, np.broadcast_to(pi[None, None, :, None], (n, nhead, l, 1)), axis=3)[..., 0]
    if s == 1:
        return float("inf")
    other = score.copy()
    np.put_along_axis(other, np.broadcast_to(pi[None, None, :, None], (n, nhead, l, 1)), -np.inf, axis=3)
    return float((win - other.max(axis=3)).min())
