"""CPU: the pure part of the wrappers' sample-form helper (``ops._sample_form`` / ``_sample_count`` / ``_sample_forms``) and the
depth-hypothesis strides (``ops._depth_strides``).  They look at shapes and strides only, so CPU tensors do; the device / dtype /
workspace check (``ops._t``) is applied separately by the wrappers."""
import pytest
import torch

from effi_mvs_plus_amd import ops


def test_unbatched_rank_is_one_item():
    assert ops._sample_form(torch.zeros(2, 3, 4), 3, "x") == (None, 0)
    assert ops._sample_form(torch.zeros(5), 1, "x") == (None, 0)


def test_batch_has_the_item_size_as_stride():
    assert ops._sample_form(torch.zeros(3, 2, 3, 4), 3, "x") == (3, 24)


def test_slice_of_a_larger_allocation_keeps_its_own_stride():
    big = torch.zeros(6, 2, 3, 4)
    assert ops._sample_form(big[::2], 3, "x") == (3, 48)
    assert ops._sample_form(big[1:4, 1:], 3, "x") == (3, 24)           # items contiguous, 12 floats each, 24 apart


def test_expanded_leading_dimension_is_shared():
    assert ops._sample_form(torch.zeros(2, 3, 4).unsqueeze(0).expand(3, 2, 3, 4), 3, "x") == (3, 0)


def test_one_sample_has_stride_zero():
    assert ops._sample_form(torch.zeros(1, 2, 3, 4), 3, "x") == (1, 0)
    assert ops._sample_form(torch.zeros(6, 2, 3, 4)[2:3], 3, "x") == (1, 0)


def test_items_must_be_contiguous():
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(3, 2, 3, 8)[..., ::2], 3, "x")
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(2, 3, 8)[..., ::2], 3, "x")      # and so must an unbatched tensor
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(3, 2, 4, 3).transpose(-1, -2), 3, "x")


def test_wrong_rank_and_empty_batch_raise():
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(3, 4), 4, "x")                   # rank off by two
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(1, 1, 3, 2, 3, 4), 4, "x")
    with pytest.raises(ValueError):
        ops._sample_form(torch.zeros(0, 2, 3, 4), 3, "x")             # n < 1


def test_sample_counts_must_agree():
    assert ops._sample_count([None, 3, None, 3], "x") == 3
    assert ops._sample_count([None, None], "x") is None
    with pytest.raises(ValueError):
        ops._sample_count([2, None, 3], "x")
    shared, a, b = torch.zeros(2, 3, 4), torch.zeros(3, 2, 3, 4), torch.zeros(6, 2, 3, 4)[::2]
    assert ops._sample_forms([a, shared, b], 3, "x") == (3, [24, 0, 48])     # a lower-rank tensor beside them is shared
    assert ops._sample_forms([shared, shared], 3, "x") == (None, [0, 0])
    with pytest.raises(ValueError):
        ops._sample_forms([a, torch.zeros(2, 2, 3, 4)], 3, "x")


# (hypothesis stride, pixel stride, sample stride) as the two functions this one replaced returned them for D = 4, h = 2, w = 3, n = 3
D, H, W, N = 4, 2, 3, 3
DEPTH_FORMS = [
    ("[D]", None, lambda: torch.rand(D), (1, 0, 0)),
    ("[D,h,w]", None, lambda: torch.rand(D, H, W), (6, 1, 0)),
    ("[D,h,w] expanded", None, lambda: torch.rand(D, 1, 1).expand(D, H, W), (1, 0, 0)),
    ("[D,h,w] expanded from a strided column", None, lambda: torch.rand(D, 2)[:, 0].view(D, 1, 1).expand(D, H, W), (2, 0, 0)),
    ("[D,h,w] transposed (copied)", None, lambda: torch.rand(D, W, H).transpose(1, 2), (6, 1, 0)),
    ("[D] shared by a batch", N, lambda: torch.rand(D), (1, 0, 0)),
    ("[n,D]", N, lambda: torch.rand(N, D), (1, 0, 4)),
    ("[n,D] sliced", N, lambda: torch.rand(2 * N, D)[::2], (1, 0, 8)),
    ("[n,D] expanded", N, lambda: torch.rand(1, D).expand(N, D), (1, 0, 0)),
    ("[1,D]", 1, lambda: torch.rand(1, D), (1, 0, 0)),
    ("[n,D,h,w]", N, lambda: torch.rand(N, D, H, W), (6, 1, 24)),
    ("[n,D,h,w] expanded", N, lambda: torch.rand(N, D, 1, 1).expand(N, D, H, W), (1, 0, 4)),
    ("[1,D,h,w] expanded", 1, lambda: torch.rand(1, D, 1, 1).expand(1, D, H, W), (1, 0, 0)),
    ("[n,D,h,w] transposed (copied)", N, lambda: torch.rand(N, D, W, H).transpose(2, 3), (6, 1, 24)),
]


@pytest.mark.parametrize("name,n,make,want", DEPTH_FORMS, ids=[f[0] for f in DEPTH_FORMS])
def test_depth_strides(name, n, make, want):
    src = make()
    depth, dds, dps, dss = ops._depth_strides(src, n, D, H, W)
    assert (dds, dps, dss) == want
    assert torch.equal(depth, src)                                   # the silent copy of a form the kernels cannot stride over
    if "copied" in name:
        assert depth.is_contiguous() and depth.data_ptr() != src.data_ptr()
    else:
        assert depth.data_ptr() == src.data_ptr()


@pytest.mark.parametrize("shape", [(N, D + 1), (D + 1,), (N, D, H, W + 1), (N, D, H + 1, W), (N + 1, D), (N + 1, D, H, W), (N, 2, 2)])
def test_batched_depth_forms_are_checked(shape):
    with pytest.raises(ValueError):
        ops._depth_strides(torch.rand(*shape), N, D, H, W)
