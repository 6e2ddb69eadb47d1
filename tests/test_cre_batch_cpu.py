"""CPU: the reference of the batched CREStereo tests (tests/test_gpu_cre_batch.py) is the batched call of the oracle.  These two
tests state what that use relies on: the oracle computes every sample of a batch as it computes that sample alone (so the
B = 1 pin of tests/test_oracle_cre.py against the imported reference covers the batched call), and the samples of every case
differ from each other by far more than the parity bar, so that a result computed from the wrong sample cannot pass."""
import pytest
import torch

import cre_batch_cases as cb


@pytest.mark.parametrize("name", ["b2_104x168_it4", "b3_72x104_it2"])
def test_batched_oracle_equals_per_sample_oracle(cre_sd, name):
    """Every output of the batched oracle call against the oracle called on each sample alone.  Nothing in the oracle mixes samples
    (instance norm, the attention sums and the samplers are per sample), but oneDNN / ATen may tile a convolution or a matmul over
    another batch size in another summation order: measured with 8 threads 9e-8 ... 1.9e-6 per output at 2 x 104x168, 7e-8 ... 8.3e-7
    at 3 x 72x104 (and 2e-7 ... 2.4e-6 at 2 x 128x192) on flows up to 5.5 / 2.2 / 6.1 px.  Bound 1e-5: room for another thread count's
    order, four orders of magnitude below what one swapped sample gives (test_samples_of_a_case_differ)."""
    from oracle import cre_ref as C
    B, H, W, iters = cb.CASES[name]
    f1, f2 = cb.frames(name)
    batched = cb.oracle(cre_sd, name)
    assert [tuple(o.shape) for o in batched] == cb.output_shapes(name)
    errs = [0.0] * len(batched)
    for i in range(B):
        single = C.cre_stereo_forward(cre_sd, f1[i:i + 1], f2[i:i + 1], iters)
        assert len(single) == len(batched)
        errs = [max(e, (b[i:i + 1] - s).abs().max().item()) for e, b, s in zip(errs, batched, single)]
    print(f"\ncre oracle {name}: batched vs per-sample max-abs per output:", " ".join(f"{e:.1e}" for e in errs),
          f"(|flow| max {batched[-1].abs().max():.1f})")
    assert max(errs) <= 1e-5


@pytest.mark.parametrize("name", list(cb.CASES))
def test_samples_of_a_case_differ(cre_sd, name):
    """A condition on the inputs, not a measurement: the final flows of any two samples of a case are more than 0.5 px apart
    (max-abs, the norm of the parity checks) in the oracle, so a kernel that reads or writes another sample's data misses the 1e-4
    bar by orders of magnitude.  A seed that stops meeting this is to be replaced, not the bound."""
    B = cb.CASES[name][0]
    last = cb.oracle(cre_sd, name)[-1]
    dist = {(i, j): (last[i] - last[j]).abs().max().item() for i in range(B) for j in range(i + 1, B)}
    print(f"\ncre oracle {name}: final-flow distance between samples:", " ".join(f"{i}-{j}: {d:.2f} px" for (i, j), d in dist.items()))
    assert min(dist.values()) > 0.5
    assert torch.isfinite(last).all()
