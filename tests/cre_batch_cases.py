"""The batched CREStereo cases that tests/test_cre_batch_cpu.py and tests/test_gpu_cre_batch.py share: sample i of a case is
weightgen.synthetic_frames(40 + i, 1, H, W) (another noise field and another shift per seed), the samples concatenated; the
reference is the batched call of oracle.cre_ref.cre_stereo_forward, computed once per case and handed out read-only."""
import torch

SEED0 = 40

# name -> (B, H, W, iters).  1/8, 1/16 and 1/32 maps: 13x21, 6x10, 3x5 (ragged at every level, odd pooling tails, W % 4 != 0 at
# 1/8 and 1/32: the scalar window kernel) | 9x13, 4x6, 2x3 | 16x24, 8x12, 4x6 (W % 4 == 0 everywhere: the 4-pixels-per-lane kernel)
CASES = {"b2_104x168_it4": (2, 104, 168, 4), "b3_72x104_it2": (3, 72, 104, 2), "b2_128x192_it4": (2, 128, 192, 4)}


def frames_of(seeds, H, W):
    """(frame1, frame2), each (len(seeds), 3, H, W): one independently generated pair per seed."""
    from nndepth_amd import weightgen
    pairs = [weightgen.synthetic_frames(s, 1, H, W) for s in seeds]
    return torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])


def frames(name):
    B, H, W, _ = CASES[name]
    return frames_of(range(SEED0, SEED0 + B), H, W)


def output_shapes(name):
    """Shapes of the 2 * iters outputs: iters // 2 of the 1/32 stage and of the 1/16 stage and iters of the 1/8 stage, each 8 x its
    stage's map (cre_stereo/model.py:221-284)."""
    B, H, W, iters = CASES[name]
    h, w = -(-H // 8), -(-W // 8)
    return ([(B, 2, 8 * (h // 4), 8 * (w // 4))] * (iters // 2) + [(B, 2, 8 * (h // 2), 8 * (w // 2))] * (iters // 2)
            + [(B, 2, 8 * h, 8 * w)] * iters)


_ORACLE = {}


def oracle(cre_sd, name):
    """Every up_disp (B,2,H,W) of the batched oracle call on frames(name), as a tuple; computed once per case (the state dict is
    the session's `cre_sd` fixture).  Callers must not write into the tensors."""
    if name not in _ORACLE:
        from oracle import cre_ref as C
        f1, f2 = frames(name)
        _ORACLE[name] = tuple(C.cre_stereo_forward(cre_sd, f1, f2, CASES[name][3]))
    return _ORACLE[name]


def per_sample_errors(got, exp):
    """max-abs of got - exp per sample of the batch, as floats."""
    return [(g - e).abs().max().item() for g, e in zip(got, exp)]
