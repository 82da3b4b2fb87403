"""CPU: the float64 clip + AdamW reference agrees with PyTorch, the optimizer's symbols are declared and exported, and
the chunk table covers every element of every tensor exactly once without crossing a tensor."""

import numpy as np
import pytest
import torch

from optim_reference import ClipAdamWReference

OPTIM_SYMBOLS = ("ud_optim_chunk_elems", "ud_optim_sqnorm", "ud_optim_clip_adamw")


def test_reference_agrees_with_torch_in_float64():
    """5 steps against clip_grad_norm_ + AdamW(foreach=True) on the CPU in float64, to 1e-12 relative; the gradient
    norms straddle max_norm so that clipping is active in steps 1, 3, 5 and inactive in steps 2, 4."""
    rng = np.random.default_rng(0)
    shapes = [(1,), (5,), (64,), (7, 9), (16, 8, 3, 3), (1000,)]
    lr, betas, eps, wd, max_norm = 2e-4, (0.9, 0.999), 1e-8, 1e-7, 0.1
    init = [rng.standard_normal(s) for s in shapes]
    params = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in init]
    opt = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=True)
    ref = ClipAdamWReference(init, lr, betas, eps, wd, max_norm)
    clipped = []
    for norm in (0.5, 0.03, 2.0, 0.05, 0.2):
        grads = [rng.standard_normal(s) for s in shapes]
        scale = norm / np.sqrt(sum((g * g).sum() for g in grads))
        grads = [g * scale for g in grads]
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g, dtype=torch.float64)
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=True)
        opt.step()
        ref.step(grads)
        clipped.append(ref.coef < 1.0)
        assert abs(float(total) - ref.total_norm) <= 1e-12 * ref.total_norm
        for i, p in enumerate(params):
            st = opt.state[p]
            for got, want in ((p.detach().numpy(), ref.p[i]), (st["exp_avg"].numpy(), ref.m[i]),
                              (st["exp_avg_sq"].numpy(), ref.v[i])):
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
            assert float(st["step"]) == ref.step_count
    assert clipped == [True, False, True, False, True]


def test_reference_skip_rule():
    ref = ClipAdamWReference([np.ones(4)], 1e-3, max_norm=0.1)
    ref.step([np.array([1.0, np.inf, 0.0, 0.0])])
    assert ref.skipped == 1 and ref.step_count == 0 and np.array_equal(ref.p[0], np.ones(4)) and not ref.m[0].any()
    ref.step([np.array([1.0, np.nan, 0.0, 0.0])])
    assert ref.skipped == 2 and ref.step_count == 0
    ref.step([None])
    assert ref.skipped == 2 and ref.step_count == 1 and ref.total_norm == 0.0
    loose = ClipAdamWReference([np.ones(4)], 1e-3, max_norm=0.1, skip_nonfinite=False)
    loose.step([np.array([1.0, np.inf, 0.0, 0.0])])
    assert not np.isfinite(loose.p[0]).all()


def test_optim_symbols_declared_and_exported(hip_lib):
    from unidistill_amd import _lib
    declared = _lib.exported_symbols()      # the prototypes parsed from unidistill_hip.h (test_abi.py counts them independently)
    for n in OPTIM_SYMBOLS:
        assert n in declared, f"{n} not declared in unidistill_hip.h"
        assert hasattr(hip_lib, n), f"{n} declared in unidistill_hip.h but not exported"
    chunk = hip_lib.ud_optim_chunk_elems()
    assert chunk >= 1024 and chunk % 1024 == 0     # 256 threads x float4


def test_launchers_reject_bad_arguments_without_a_gpu(hip_lib):
    assert hip_lib.ud_optim_sqnorm(None, 1, None, None, None, None) == -1
    assert hip_lib.ud_optim_clip_adamw(None, 1, None, None, None, None, None, None, 0.9, 0.999, 1e-8, 0.0, 0.1, 1, None) == -1
    assert hip_lib.ud_error_string(-1).decode() == "invalid argument"


def _sizes(chunk):
    return [1, 3, 4, 5, 63, 64, 65, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 16 * 8 * 3 * 3, 8 * 4, 1001, 0]


@pytest.mark.parametrize("chunk", [8, 1024, 65536])
def test_chunk_table_covers_every_element_once(chunk):
    from unidistill_amd.ops.optim import build_chunk_table
    sizes = _sizes(chunk)
    table = build_chunk_table(sizes, chunk)
    assert len(table) == sum((n + chunk - 1) // chunk for n in sizes)
    assert table.dtype.itemsize == 16
    cover = [np.zeros(n, dtype=np.int32) for n in sizes]
    for rec in table:
        t, off, length = int(rec["tensor"]), int(rec["offset"]), int(rec["length"])
        assert 0 <= t < len(sizes) and 1 <= length <= chunk and off % chunk == 0
        assert off + length <= sizes[t], "chunk crosses the end of its tensor"
        assert length == chunk or off + length == sizes[t], "only a tensor's last chunk may be short"
        cover[t][off:off + length] += 1
    assert all((c == 1).all() for c in cover)
    assert np.array_equal(table["tensor"], np.sort(table["tensor"]))


def test_chunk_table_uses_the_library_chunk_size(hip_lib):
    from unidistill_amd.ops import optim
    assert optim.chunk_elems() == hip_lib.ud_optim_chunk_elems()
    big = build = optim.build_chunk_table([2 ** 31 + 5], optim.chunk_elems())      # offsets past 2^31 stay exact
    assert int(build["offset"][-1]) + int(big["length"][-1]) == 2 ** 31 + 5
    with pytest.raises(ValueError):
        optim.build_chunk_table([-1], 8)


def test_no_cpu_fallback(hip_lib):
    from unidistill_amd.ops.optim import ClipAdamW
    with pytest.raises(RuntimeError, match="GPU only"):
        ClipAdamW([torch.zeros(4, requires_grad=True)], lr=1e-3)
