"""The checked handle `_lib.ud` on the GPU: tensors in place of data_ptr()s launch the same kernel with the same bits, a rejected
argument raises, and a temporary passed inline lives until the call has returned."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(64, 32, generator=g).cuda()
    scale = (torch.rand(32, generator=g) + 0.5).cuda()
    shift = torch.randn(32, generator=g).cuda()
    return x, scale, shift


def test_checked_call_equals_raw_call(hip_lib):
    from unidistill_amd import _lib
    x, scale, shift = _case()
    s = _lib.stream_of(x)
    raw, chk = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    assert hip_lib.ud_bn_act_fwd_f32(x.data_ptr(), None, scale.data_ptr(), shift.data_ptr(), raw.data_ptr(), 64, 32, 1, s) == 0
    assert _lib.ud.ud_bn_act_fwd_f32(x, None, scale, shift, chk, 64, 32, 1, s) == 0
    torch.cuda.synchronize()
    ref = torch.relu(x.double() * scale.double() + shift.double())
    assert ref.max() < 16 and (raw.double() - ref).abs().max() <= 1e-6      # at most two fp32 roundings below 16: 2 * 2^-21
    assert not torch.isnan(chk).any() and torch.equal(raw.view(torch.int32), chk.view(torch.int32))


def test_checked_call_raises_on_a_rejected_argument(hip_lib):
    """A leading dimension that is no multiple of 8: refused by the launcher's argument check, before any launch."""
    from unidistill_amd import _lib
    x, scale, shift = _case()
    y = torch.zeros(64, 64, device="cuda")
    s = _lib.stream_of(x)
    code = hip_lib.ud_bn_act_fwd_ld_f32(x.data_ptr(), None, scale.data_ptr(), shift.data_ptr(), y.data_ptr(), 64, 32, 36, 1, s)
    assert code != 0
    with pytest.raises(RuntimeError, match=rf"ud_bn_act_fwd_ld_f32 failed: .* \({code}\)"):
        _lib.ud.ud_bn_act_fwd_ld_f32(x, None, scale, shift, y, 64, 32, 36, 1, s)
    torch.cuda.synchronize()
    assert not y.any()


def test_inline_temporary_is_kept_until_the_call_returns(hip_lib):
    from unidistill_amd import _lib
    x, scale, shift = _case()
    s = _lib.stream_of(x)
    named, inline = torch.empty_like(x), torch.empty_like(x)
    _lib.ud.ud_bn_act_fwd_f32(x, None, scale, shift, named, 64, 32, 1, s)
    _lib.ud.ud_bn_act_fwd_f32(x.clone(), None, scale.clone(), shift.clone(), inline, 64, 32, 1, s)
    torch.cuda.synchronize()
    assert torch.equal(named.view(torch.int32), inline.view(torch.int32))
