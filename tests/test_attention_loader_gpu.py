"""GPU: the K / V^T tile loader of ``attention_kernel`` (csrc/tg_attention.hip).  Full key tiles of segment 0 are staged from running source pointers
(``issue_full``); ragged tiles, causal launches and segment 1 from the generic ``issue``.  The cases (tests/golden/make_attention_parent.py) walk every
order in which the two alternate — one full tile, several (both LDS stages), full tiles then a ragged one, then segment 1, ragged only, causal — at one,
two and three K panels, in the instances with and without the bias fold, the ones row and the mask, in a layout whose padding is NaN: K inside a fused
buffer (pitch 2 C, gap rows between batch items), V^T rows with 8 to 15 spare columns.

 * ``test_against_fp64``: an fp64 restatement of the contract, with the tolerance helper and scale of ``test_attention`` (tests/test_kernels_gpu.py).
 * ``test_bit_identical_to_the_parent_kernel``: tests/golden/attention_parent.npz holds the output bits of the parent commit's library on an MI355X; the
   loader moves bytes and no arithmetic changed, so every bit must match.

The same two checks for ``tg_attention_wide`` (with its key split) and ``tg_attention_relpos`` against tests/golden/attention_parent_wide_relpos.npz: the
three kernels share their tile machinery (csrc/tg_attn_fwd.h), and the file holds what each computed when it still carried its own copy.
"""
import functools

import numpy as np
import pytest
import torch

from tests.golden import make_attention_parent as gen
from tests.test_kernels_gpu import check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, fp64 reference): computed once per case, shared by both dtypes and both tests, never written to"""
    inp = gen.make_inputs(name)
    return inp, gen.reference(name, inp)


@functools.lru_cache(maxsize=None)
def _output(name, tag):
    from theatergen_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return gen.run(ops, name, _case(name)[0], gen.DTYPES[tag], DEV).cpu()


@pytest.fixture(scope="module")
def gold():
    z = np.load(gen.PATH)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", list(gen.DTYPES))
@pytest.mark.parametrize("name", list(gen.CASES))
def test_against_fp64(name, tag):
    check(_output(name, tag), _case(name)[1], gen.DTYPES[tag], f"attention loader {name} {tag}", scale=1.5)


@pytest.mark.parametrize("tag", list(gen.DTYPES))
@pytest.mark.parametrize("name", list(gen.CASES))
def test_bit_identical_to_the_parent_kernel(gold, name, tag):
    assert np.array_equal(gen.inputs_digest(_case(name)[0]), gold[f"{name}/inputs_sha256"]), f"{name}: the generated inputs are not the recorded ones"
    got, want = _output(name, tag).view(torch.int16).numpy(), gold[f"{name}/{tag}"]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), f"{name} {tag}: differs from the parent's in {int((got != want).sum())} of {want.size} values"


# ---- tg_attention_wide, tg_attention_relpos --------------------------------------------------------------------------------------------------------------
CASES2 = list(gen.WIDE_CASES) + list(gen.RELPOS_CASES)


@functools.lru_cache(maxsize=None)
def _case2(name):
    inp = gen.make_inputs2(name)
    return inp, gen.reference2(name, inp)


@functools.lru_cache(maxsize=None)
def _output2(name, tag):
    from theatergen_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return gen.run2(ops, name, _case2(name)[0], gen.DTYPES[tag], DEV).cpu()


@pytest.fixture(scope="module")
def gold2():
    z = np.load(gen.PATH_WIDE_RELPOS)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("tag", list(gen.DTYPES))
@pytest.mark.parametrize("name", CASES2)
def test_wide_relpos_against_fp64(name, tag):
    check(_output2(name, tag), _case2(name)[1], gen.DTYPES[tag], f"attention {name} {tag}", scale=1.5)


@pytest.mark.parametrize("tag", list(gen.DTYPES))
@pytest.mark.parametrize("name", CASES2)
def test_wide_relpos_bit_identical_to_the_parent_kernel(gold2, name, tag):
    assert np.array_equal(gen.inputs_digest(_case2(name)[0]), gold2[f"{name}/inputs_sha256"]), f"{name}: the generated inputs are not the recorded ones"
    got, want = gen.stored_form(_output2(name, tag)), gold2[f"{name}/{tag}"]           # one SHA-256 per (batch item, block of 128 queries)
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = [(b, i) for b in range(want.shape[0]) for i in range(want.shape[1]) if not np.array_equal(got[b, i], want[b, i])]
    assert not bad, f"{name} {tag}: (batch item, query block) {bad} differ from the parent's"
