"""CPU: fp16x2 activation ranges as data (include/nndepth_amd.h "fp16x2 activation range": nnd_*_scale_slots, nnd_scales_read /
nnd_scales_write, nnd_nonfinite_flag; raft_stereo.calibration_state and friends; parallel.sync_calibration).
  a. slot enumeration of the four engine kinds — host functions: counts, names, -1 where a layer has no scale, NULL sizing, a too
     small array refused — and that every offset points at a slot of a freshly packed blob ({2^-(s+2), 4, 0, 2^-s})
  b. the state of the model classes: format, keys from the structure, what load_calibration_state refuses, pending states
  c. sync_calibration in a gloo world of 2
Nothing here needs a GPU: a state loaded without one stays pending."""
import ctypes as C
import json
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ENC_NAMES = (["conv1"] + [f"{b}.{c}" for b in ("layer1.0", "layer1.1", "layer2.0", "layer2.1", "layer3.0", "layer3.1")
                          for c in ("conv1", "conv2", "downsample.0")] + ["conv2", "cnet_proj"])


def _offsets(call, n):
    offs = (C.c_int64 * n)(*([-7] * n))
    return call(offs, n), list(offs)


def _is_fresh_slot(blob, off):
    """{oscale, xscale, record, wsinv} of a layer nobody calibrated: xs = 2, oscale = wsinv / 4, no record."""
    o, x, a, w = (float(v) for v in blob[off:off + 4])
    return x == 4.0 and a == 0.0 and w > 0 and o == w / 4.0


# ------------------------------------------------------------------------------------------------ a. slot enumeration
@pytest.mark.parametrize("cnet_dim", [0, 192])
@pytest.mark.parametrize("norm", ["batch", "instance"])
def test_encoder_scale_slots(raft_sd, norm, cnet_dim):
    from nndepth_amd import ops
    from nndepth_amd._lib import lib
    eng = ops.EncoderEngine(256, norm, cnet_dim, "fp16x2")
    d = C.byref(eng.desc)
    n = lib.nnd_encoder_scale_slots(d, None, 0)  # NULL sizes the array
    assert n == 20 + (cnet_dim > 0)
    assert [lib.nnd_encoder_scale_name(d, i).decode() for i in range(n)] == ENC_NAMES[:n]
    assert lib.nnd_encoder_scale_name(d, n) == b"" and lib.nnd_encoder_scale_name(d, -1) == b""
    rc, offs = _offsets(lambda o, k: lib.nnd_encoder_scale_slots(d, o, k), n)
    assert rc == n
    # exact fp32 inside an fp16x2 encoder: the stem, conv2 and the stand-in shortcuts of the four stride-1 blocks
    no_scale = {"conv1", "conv2", "layer1.0.downsample.0", "layer1.1.downsample.0", "layer2.1.downsample.0", "layer3.1.downsample.0"}
    assert {ENC_NAMES[i] for i in range(n) if offs[i] < 0} == no_scale and all(o == -1 for o in offs if o < 0)
    assert eng.scale_names() == [ENC_NAMES[i] for i in range(n) if offs[i] >= 0]
    rc, _ = _offsets(lambda o, k: lib.nnd_encoder_scale_slots(d, o, k), n - 1)  # too small: refused, nothing half-filled silently
    assert rc == -1 and b"encoder_scale_slots" in lib.nnd_last_error()
    # every offset is a slot of the packed blob
    enc_sd = {k[len("fnet."):]: v for k, v in raft_sd.items() if k.startswith("fnet.") and (norm == "batch" or "norm" not in k)}
    cnet_sd = {k[len("cnet_proj."):]: v for k, v in raft_sd.items() if k.startswith("cnet_proj.")}
    blob = eng.load(enc_sd, cnet_sd if cnet_dim else None, device="cpu").packed
    assert len({o for o in offs if o >= 0}) == len(eng.scale_names())
    for o in offs:
        assert o < 0 or (o + 4 <= blob.numel() and _is_fresh_slot(blob, o)), o
    for arithmetic in ("fp32", "bf16x3"):
        e2 = ops.EncoderEngine(256, norm, cnet_dim, arithmetic)
        rc, offs = _offsets(lambda o, k: lib.nnd_encoder_scale_slots(C.byref(e2.desc), o, k), n)
        assert rc == n and offs == [-1] * n and e2.scale_names() == []
    assert ops.EncoderEngine(256, norm, cnet_dim, "fp16").scale_names() == eng.scale_names()  # one piece: the same scales


@pytest.mark.parametrize("gru", ["sep_conv", "conv_gru"])
def test_update_block_scale_names(gru):
    from nndepth_amd import ops
    from nndepth_amd._lib import lib
    eng = ops.UpdateBlockEngine(128, 64, 36, 1, 576, gru, "fp16x2")
    n = lib.nnd_update_block_scale_slots(C.byref(eng.desc), None, 0)
    rc, offs = _offsets(lambda o, k: lib.nnd_update_block_scale_slots(C.byref(eng.desc), o, k), n)
    names = eng.scale_names()
    assert rc == n == 18 and len(set(names)) == len(names) == len({o for o in offs if o >= 0})
    assert "encoder.convc2" in names and "mask.2" in names and "encoder.convc1" not in names  # 36 planes: not a multiple of 16
    assert ("gru.convq2[rh,motion]" in names) == (gru == "sep_conv")  # conv_gru: the second pass aliases the first, listed once
    for arithmetic in ("fp32", "bf16x3"):
        assert ops.UpdateBlockEngine(128, 64, 36, 1, 576, gru, arithmetic).scale_names() == []
    assert ops.UpdateBlockEngine(64, 64, 576, 1, 144, gru, "fp16x2").scale_names()[0] == "encoder.convc1"  # IGEV's 576 planes


def test_conv3d_scale_slots():
    """A thin stride-1 layer packs three formulations of itself, a wide one the plain one alone; every slot is found in the blob."""
    from nndepth_amd import ops
    from nndepth_amd._lib import lib, Conv3dDesc
    assert [lib.nnd_conv3d_scale_name(i) for i in (-1, 0, 1, 2, 3)] == [b"", b"plain", b"grouped", b"slab", b""]
    g = torch.Generator().manual_seed(0)
    for (cout, cin, stride), want in {(16, 16, 1): ["plain", "grouped", "slab"], (32, 32, 1): ["plain"], (16, 48, 1): ["plain", "grouped"],
                                      (16, 8, 2): ["slab"]}.items():
        w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05
        bn = (torch.ones(cout), torch.zeros(cout), torch.zeros(cout), torch.ones(cout))
        conv = ops.Conv3dNorm(w, None, stride, bn, 1e-5, 0.01, 0, "cpu", arithmetic="fp16x2")
        d = C.byref(conv.desc)
        assert lib.nnd_conv3d_scale_slots(d, None, 0) == 3
        rc, offs = _offsets(lambda o, k: lib.nnd_conv3d_scale_slots(d, o, k), 3)
        assert rc == 3 and [n for n, o in zip(("plain", "grouped", "slab"), offs) if o >= 0] == want
        assert all(o == -1 for o in offs if o < 0)
        assert [n for n, _ in conv.formulations()] == want and conv.scale_names() == [""]  # ONE layer, whatever it packs
        for o in offs:
            assert o < 0 or (o + 4 <= conv.packed.numel() and _is_fresh_slot(conv.packed, o)), (cout, cin, stride, o)
        rc, _ = _offsets(lambda o, k: lib.nnd_conv3d_scale_slots(d, o, k), 2)
        assert rc == -1 and b"conv3d_scale_slots" in lib.nnd_last_error()
        for arithmetic in (0, 3):
            d2 = Conv3dDesc(cout, cin, 0, stride, arithmetic, 0)
            assert _offsets(lambda o, k: lib.nnd_conv3d_scale_slots(C.byref(d2), o, k), 3) == (3, [-1, -1, -1])
            assert ops.Conv3dNorm.formulations_of(d2) == []


def test_conv2d_scale_slot():
    from nndepth_amd import ops
    from nndepth_amd._lib import lib
    conv = ops.Conv2d(torch.randn(48, 32, 3, 3), torch.zeros(48), device=None, arithmetic="fp16x2")
    assert lib.nnd_conv2d_scale_slots_ex(48, 32, 3, 3, 2, None, 0) == 1
    rc, offs = _offsets(lambda o, k: lib.nnd_conv2d_scale_slots_ex(48, 32, 3, 3, 2, o, k), 1)
    assert rc == 1 and offs[0] == conv.packed_host.numel() - 4 and _is_fresh_slot(conv.packed_host, offs[0])
    assert conv.scale_names() == [""]
    # "fp16" (one piece, half the weight bytes): a slot as well, at the end of ITS blob
    assert _offsets(lambda o, k: lib.nnd_conv2d_scale_slots_ex(48, 32, 3, 3, 1, o, k), 1) == (1, [lib.nnd_conv2d_packed_floats_ex(48, 32, 3, 3, 1) - 4])
    for arithmetic in (0, 3):
        assert _offsets(lambda o, k: lib.nnd_conv2d_scale_slots_ex(48, 32, 3, 3, arithmetic, o, k), 1) == (1, [-1])
    rc, _ = _offsets(lambda o, k: lib.nnd_conv2d_scale_slots_ex(48, 32, 3, 3, 2, o, 0), 1)
    assert rc == -1 and b"conv2d_scale_slots" in lib.nnd_last_error()
    assert lib.nnd_conv2d_scale_slots_ex(48, 32, 7, 7, 2, None, 0) == -1  # a kernel size that is not built
    with pytest.raises(ops.NndError, match="not packed on a HIP device"):
        conv.read_scales()


def test_scales_entry_points_validate_their_arguments():
    """Refused before anything is launched: the pointers below are never dereferenced."""
    from nndepth_amd._lib import lib
    p = C.c_void_p(64)  # stands for a device pointer
    one, two_same, negative = (C.c_int64 * 1)(8), (C.c_int64 * 2)(8, 8), (C.c_int64 * 2)(8, -1)

    def refused(rc, word):
        assert rc == -1 and word in lib.nnd_last_error(), (rc, lib.nnd_last_error())

    refused(lib.nnd_scales_read(None, one, 1, p, None, 0, None), b"null")
    refused(lib.nnd_scales_read(p, None, 1, p, None, 0, None), b"null")
    refused(lib.nnd_scales_read(p, one, 1, None, None, 0, None), b"null")
    refused(lib.nnd_scales_read(p, one, 0, p, None, 0, None), b"n = 0")
    refused(lib.nnd_scales_read(p, one, 65, p, None, 0, None), b"n = 65")
    refused(lib.nnd_scales_read(p, negative, 2, p, None, 0, None), b"offset -1")
    refused(lib.nnd_scales_write(None, one, 1, p, 0, None), b"null")
    refused(lib.nnd_scales_write(p, one, 1, None, 0, None), b"null")
    refused(lib.nnd_scales_write(p, one, -1, p, 0, None), b"n = -1")
    refused(lib.nnd_scales_write(p, one, 1, p, 2, None), b"mode 2")
    refused(lib.nnd_scales_write(p, two_same, 2, p, 1, None), b"the same")
    refused(lib.nnd_scales_write(p, negative, 2, p, 0, None), b"offset -1")
    refused(lib.nnd_nonfinite_flag(None, 4, p, None), b"null")
    refused(lib.nnd_nonfinite_flag(p, 4, None, None), b"null")
    refused(lib.nnd_nonfinite_flag(p, 0, p, None), b"n = 0")
    refused(lib.nnd_nonfinite_flag(p, -3, p, None), b"n = -3")


# --------------------------------------------------------------------------------------------------- b. the state
def _make(name, arithmetic="fp16x2"):
    """The small models of tests/test_gpu_calib.py, on the host."""
    if name == "raft":
        from nndepth_amd.raft_stereo import BaseRAFTStereo
        return BaseRAFTStereo(iters=6, context_dim=64, arithmetic=arithmetic).eval()
    if name == "cre":
        from nndepth_amd.cre_stereo import CREStereoBase
        return CREStereoBase(iters=4, arithmetic=arithmetic).eval()
    if name == "igev":
        from igev_double import make_igev
        from nndepth_amd.igev_stereo import CostVolumeFilterNetwork, IGEVStereoBase
        return make_igev(IGEVStereoBase, CostVolumeFilterNetwork, iters=4, hidden_dim=64, context_dim=64, arithmetic=arithmetic).eval()
    from c2f_double import make_c2f
    from nndepth_amd.raft_stereo import Coarse2FineRAFTStereoBase
    return make_c2f(Coarse2FineRAFTStereoBase, iters=3, corr_levels=1, arithmetic=arithmetic).eval()


def _raft():
    return _make("raft")


MODELS = ("raft", "cre", "igev", "c2f")


def _keys(model):
    from nndepth_amd.raft_stereo import calibration_sites
    return [f"{p}/{n}" if n else p for p, s in calibration_sites(model).items() for n in s.names]


def _state(model, value=lambda i: 3, arithmetic="fp16x2"):
    return {"version": 1, "arithmetic": arithmetic, "layers": {k: value(i) for i, k in enumerate(_keys(model))}}


@pytest.mark.parametrize("name", list(MODELS))
def test_state_keys_come_from_module_paths_and_state_dict_is_untouched(name, tmp_path):
    m = _make(name)
    keys = _keys(m)
    assert len(set(keys)) == len(keys) and "update_block/encoder.convc2" in keys
    assert ("fnet/layer1.0.conv1" in keys) == (name in ("raft", "cre")) and ("fnet/cnet_proj" in keys) == (name == "raft")
    assert ("cv_regularizer.conv1.0" in keys and "cv_regularizer.final_conv" in keys) == (name == "igev")
    sd_keys = list(m.state_dict())
    st = _state(m, lambda i: 5 - i % 9)
    assert m.load_calibration_state(json.loads(json.dumps(st))) is m  # JSON round trip; no GPU: the state stays pending ...
    assert m.calibration_state() == st and m.calibration_state() is not st  # ... and is what calibration_state() returns
    assert list(m.state_dict()) == sd_keys  # reference checkpoints keep loading with strict=True
    m.load_state_dict(_make(name).state_dict(), strict=True)
    m.save_calibration(str(tmp_path / "calib.json"))
    other = _make(name)
    assert other.load_calibration(str(tmp_path / "calib.json")).calibration_state() == st
    torch.save(st, str(tmp_path / "calib.pt"))
    assert torch.load(str(tmp_path / "calib.pt")) == st
    from nndepth_amd._lib import NndError
    with pytest.raises(NndError, match="not packed yet"):
        m.clear_calibration_state().calibration_state()
    for arithmetic in ("fp32", "bf16x3"):  # nothing to calibrate: an empty state
        assert _keys(_make(name, arithmetic)) == []


def test_keys_do_not_depend_on_the_order_in_which_engines_are_built():
    """Three instances: encoder packed first, update block packed first, nothing packed (host packs: no GPU)."""
    a, b, c = _raft(), _raft(), _raft()
    a._encoder_engine("cpu"), a.update_block.sync_engine("cpu")
    b.update_block.sync_engine("cpu"), b._encoder_engine("cpu")
    assert _keys(a) == _keys(b) == _keys(c)
    st = _state(c, lambda i: i % 7 - 3)
    for m in (a, b, c):  # engines packed on the host are not written: the state is pending for them too
        assert m.load_calibration_state(st).calibration_state() == st
    assert a.update_block._packed.on_build is not None and a._enc_cache.on_build is not None
    a.update_block.encoder.convc2.weight.data.mul_(1.0)  # a repack re-applies the pinned state through the cache's hook
    a.update_block.sync_engine("cpu")
    a.clear_calibration_state()
    assert a.update_block._packed.on_build is None and a._enc_cache.on_build is None


def test_load_calibration_state_names_what_it_refuses():
    from nndepth_amd._lib import NndError
    m = _raft()
    good = _state(m)
    missing = {**good, "layers": {k: v for k, v in good["layers"].items() if k != "fnet/layer2.0.downsample.0"}}
    with pytest.raises(NndError, match=r"missing: fnet/layer2\.0\.downsample\.0"):
        m.load_calibration_state(missing)
    extra = {**good, "layers": {**good["layers"], "update_block/gru.convz9": 1}}
    with pytest.raises(NndError, match=r"unexpected: update_block/gru\.convz9"):
        m.load_calibration_state(extra)
    both = {**good, "layers": {**missing["layers"], "fnet/conv1": 2}}
    with pytest.raises(NndError, match=r"missing: fnet/layer2\.0\.downsample\.0; unexpected: fnet/conv1"):
        m.load_calibration_state(both)
    with pytest.raises(NndError, match="arithmetic 'fp16'.*runs 'fp16x2'"):
        m.load_calibration_state({**good, "arithmetic": "fp16"})
    with pytest.raises(NndError, match="version 1"):
        m.load_calibration_state({**good, "version": 2})
    for bad in (61, 2.0, True, "3"):
        with pytest.raises(NndError, match="update_block/mask.2.*-60 .. 60"):
            m.load_calibration_state({**good, "layers": {**good["layers"], "update_block/mask.2": bad}})
    assert m._calib_pinned is None  # a refused state leaves nothing behind
    with pytest.raises(NndError, match="missing"):  # another model's state: by name as well
        m.load_calibration_state(_state(_make("c2f")))


def test_patched_reference_model_has_the_same_functions():
    """patch() on a module that only has the reference's seams: the state covers the update block, the one HIP engine it installs."""
    from nndepth_amd import raft_stereo as RS
    from nndepth_amd.blocks import BasicUpdateBlock

    class Ref(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.update_block = BasicUpdateBlock(hidden_dim=128, cor_planes=36, context_dim=64, flow_channel=1, spatial_scale=8)

    m = RS.patch(Ref(), "fp16x2")
    keys = _keys(m)
    assert keys and all(k.startswith("update_block/") for k in keys)
    st = {"version": 1, "arithmetic": "fp16x2", "layers": {k: -1 for k in keys}}
    assert RS.calibration_state(RS.load_calibration_state(m, st)) == st
    with pytest.raises(RS.NndError, match="not packed yet"):
        RS.calibration_state(RS.clear_calibration_state(m))


def test_range_watch_is_off_by_default_and_reads_nothing_without_a_forward():
    m = _raft()
    assert m.watch_range is False and m.range_status() == {"overflow": False, "forwards": 0}
    m.reset_range_status()


# ------------------------------------------------------------------------------------------- c. the same ranges on every rank
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sync_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from nndepth_amd import parallel
    parallel.init_distributed("gloo")
    m = _raft()
    mine = _state(m, (lambda i: i % 5 - 2) if rank == 0 else (lambda i: 3 - i % 4))  # each rank "calibrated on its own shard"
    m.load_calibration_state(mine)
    common = parallel.sync_calibration(m)
    parallel.barrier()
    q.put((rank, mine["layers"], common, m.calibration_state()))
    dist.destroy_process_group()


def test_sync_calibration_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, a, common0, state0), (_, b, common1, state1) = res
    assert a != b and list(a) == list(b)
    want = {k: min(a[k], b[k]) for k in a}
    assert want != a and want != b  # each rank had to give way somewhere
    assert common0 == common1 == state0 == state1 == {"version": 1, "arithmetic": "fp16x2", "layers": want}


def test_sync_calibration_single_process_pins_the_own_state():
    from nndepth_amd import parallel
    m = _raft()
    st = _state(m, lambda i: i % 3)
    m.load_calibration_state(st)
    assert parallel.sync_calibration(m) == st and m.calibration_state() == st
