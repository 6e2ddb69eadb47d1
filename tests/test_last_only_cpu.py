"""CPU: the last-upsample-only mode of the refinement loops (NND_FLAG_LAST_UPSAMPLE_ONLY, `last_only=True`, `outputs="last"`) where
no GPU is needed: the flag's value, a blob layout that ignores it, the argument checks that fire before any launch, and the
validation of the Python switches."""
import ctypes as C

import pytest
import torch


def _desc(flags, arithmetic=0):
    from nndepth_amd._lib import UpdateBlockDesc
    return UpdateBlockDesc(128, 64, 36, 1, 576, 0, arithmetic, 0, flags)


def test_flag_value_and_blob_layout_independent_of_it():
    from nndepth_amd import _lib, ops, weightgen
    from nndepth_amd._lib import lib
    from oracle import torch_ref as R
    assert _lib.NND_FLAG_LAST_UPSAMPLE_ONLY == 2
    for arithmetic in (0, 3, 2):
        n0 = lib.nnd_update_block_packed_floats(C.byref(_desc(0, arithmetic)))
        assert n0 > 0
        assert lib.nnd_update_block_packed_floats(C.byref(_desc(2, arithmetic))) == n0
        assert lib.nnd_update_block_packed_floats(C.byref(_desc(3, arithmetic))) == n0  # with NND_FLAG_CALIBRATE
    assert lib.nnd_update_block_packed_floats(C.byref(_desc(8))) < 0 and b"flags" in lib.nnd_last_error()
    sd = weightgen.fill_state_dict(R.update_block_spec("u", 128, 36, 64, 1, 8))
    eng = ops.UpdateBlockEngine(128, 64, 36, 1, 576, "sep_conv", "fp16x2")
    plain = eng.pack_host(sd, "u.")
    eng.desc.flags = 2
    flagged = eng.pack_host(sd, "u.")
    eng.desc.flags = 0
    assert torch.equal(plain, flagged)


def test_refine_refuses_the_flag_with_a_stride_before_any_launch():
    from nndepth_amd._lib import lib
    d = _desc(2)
    assert lib.nnd_raft_stereo_refine(C.byref(d), None, None, 4, 4, None, None, None, None, 4096, None, None, None,
                                      1, 8, 8, 8, 4, None) < 0
    assert b"up_iter_stride" in lib.nnd_last_error()
    # (the IGEV / CREStereo entry points check their own pointers first, then run the same check in the shared loop)
    g = _desc(2)
    assert lib.nnd_raft_stereo_group_refine(C.byref(g), None, None, 1, 4, 4, None, None, None, None, 4096, None, None, None,
                                            1, 8, 8, 8, 4, None) < 0
    assert b"up_iter_stride" in lib.nnd_last_error()
    # without the flag the same call gets as far as the null pointers
    assert lib.nnd_raft_stereo_refine(C.byref(_desc(0)), None, None, 4, 4, None, None, None, None, 4096, None, None, None,
                                      1, 8, 8, 8, 4, None) < 0
    assert b"up_iter_stride" not in lib.nnd_last_error()


def test_other_entry_points_refuse_the_flag():
    from nndepth_amd._lib import lib
    d = _desc(2)
    assert lib.nnd_update_block_forward(C.byref(d), None, None, None, None, None, None, None, None, None, 1, 8, 8, None) < 0
    assert b"NND_FLAG_LAST_UPSAMPLE_ONLY" in lib.nnd_last_error()
    ms, fl = C.c_float(), C.c_double()
    assert lib.nnd_profile_conv(C.byref(d), None, None, 1, 8, 8, 8, 1, None, C.byref(ms), C.byref(fl)) < 0
    assert b"NND_FLAG_LAST_UPSAMPLE_ONLY" in lib.nnd_last_error()
    assert lib.nnd_profile_loop_conv(C.byref(d), None, None, 4, 4, None, None, None, None, 1, 8, 8, 8, 4, 8, None, C.byref(ms)) < 0
    assert b"NND_FLAG_LAST_UPSAMPLE_ONLY" in lib.nnd_last_error()


def test_model_outputs_switch():
    from nndepth_amd._lib import NndError
    from nndepth_amd.cre_stereo import CREStereoBase
    from nndepth_amd.raft_stereo import BaseRAFTStereo
    m = BaseRAFTStereo(iters=2, context_dim=64, outputs="last")
    assert m.outputs == "last" and BaseRAFTStereo(iters=2, context_dim=64).outputs == "all"
    assert set(m.state_dict()) == set(BaseRAFTStereo(iters=2, context_dim=64).state_dict())
    with pytest.raises(NndError, match="outputs"):
        BaseRAFTStereo(iters=2, context_dim=64, outputs="bogus")
    assert CREStereoBase(iters=2, outputs="last").outputs == "last"
    with pytest.raises(NndError, match="outputs"):
        CREStereoBase(iters=2, outputs="first")
    m.outputs = "every"  # set after construction: refused when the forward reads it
    x = torch.zeros(1, 3, 32, 64)
    with pytest.raises(NndError, match="outputs"):
        m.eval()(x, x)


def test_refine_last_only_arguments():
    from nndepth_amd import _lib, ops, weightgen
    from nndepth_amd._lib import NndError
    from oracle import torch_ref as R
    eng = ops.UpdateBlockEngine(128, 64, 36, 1, 576, "sep_conv", "fp16x2")
    eng.load(weightgen.fill_state_dict(R.update_block_spec("u", 128, 36, 64, 1, 8)), "u.", device="cpu")
    z = torch.zeros(1, 128, 8, 8)
    for call in (lambda **k: eng.refine(None, 4, 4, z, z, 8, 4, **k),
                 lambda **k: eng.refine_group(None, 1, 4, 4, z, z, 8, 4, **k),
                 lambda **k: eng.refine_igev(None, None, 8, 4, 4, z, z, 8, 4, **k),
                 lambda **k: eng.refine_cre(None, None, z, z, 8, 4, **k)):
        with pytest.raises(NndError, match="keep_all"):
            call(keep_all=True, last_only=True)
    # the flag is set on a per-call copy of the descriptor, never on the engine's own
    d = ops._call_desc(eng, _lib.NND_FLAG_LAST_UPSAMPLE_ONLY)
    assert d.flags == 2 and eng.desc.flags == 0
    assert ops._call_desc(eng).flags == 0
