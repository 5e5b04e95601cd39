"""Host side of the IUV / partial-IUV / loss glue (iuv_ops.py, part_ops.py, loss_ops.py): the padded-base hand-over rule, the 6-D view
unwrapping, the shared argument check and the GPU-only error -- everything that decides before a kernel runs.  No GPU needed."""
import pytest
import torch

B, S = 2, 4
WIDTHS = ((25, 32), (25, 32), (25, 32), (15, 16))


def _head(n, ld, dtype=torch.float32, first=0, base=True):
    """A [:, first:first+n] view of an NHWC [B,ld,S,S] buffer, carrying the buffer as `_padded_base` (base=False: not carrying it)."""
    b = torch.zeros(B, S, S, ld, dtype=dtype).permute(0, 3, 1, 2)
    v = b[:, first:first + n]
    if base:
        v._padded_base = b
    return v


def _same(got, want):
    return len(got) == 4 and all(g is w for g, w in zip(got, want))


def test_padded_bases_table(monkeypatch):
    from danet_densepose2smpl_amd import iuv_ops
    heads = [_head(n, ld) for n, ld in WIDTHS]
    assert _same(iuv_ops._padded_bases(*heads), [h._padded_base for h in heads])
    for k, odd in ((0, _head(25, 32, base=False)),                 # one head has no base
                   (1, _head(25, 28)),                             # one base has leading width 28
                   (3, _head(15, 16, dtype=torch.float64)),        # one base is fp64
                   (2, _head(25, 32, first=1))):                   # one view starts at channel 1: data_ptr differs
        mixed = list(heads)
        mixed[k] = odd
        assert _same(iuv_ops._padded_bases(*mixed), mixed), k
    with torch.no_grad():
        assert _same(iuv_ops._padded_bases(*heads), heads)
    monkeypatch.setattr(iuv_ops, 'PADDED_BASES', False)
    assert _same(iuv_ops._padded_bases(*heads), heads)
    monkeypatch.undo()
    assert _same(iuv_ops._padded_bases(*heads), [h._padded_base for h in heads])


def test_flat_unwraps_the_six_d_views():
    from danet_densepose2smpl_amd import part_ops
    p = torch.zeros(B, S, S, 576).permute(0, 3, 1, 2)
    assert part_ops._flat(part_ops.padded_view6(p)) is p
    v6 = torch.arange(B * 504 * 6, dtype=torch.float32).reshape(B, 24, 3, 7, 2, 3)
    flat = part_ops._flat(v6)
    assert flat.shape == (B, 504, 2, 3) and torch.equal(flat, v6.reshape(B, 504, 2, 3))
    assert part_ops._flat(flat) is flat and part_ops._flat(p) is p
    with pytest.raises(ValueError, match='must have 504 or 576 channels, got 500'):
        part_ops._flat(torch.zeros(B, 500, 2, 3))


@pytest.mark.parametrize('op', ['part_losses', 'part_joint', 'part_gt'])
def test_gt_args_cast_and_name_the_calling_op(op):
    from danet_densepose2smpl_amd import part_ops
    good = dict(iuv_img=torch.zeros(B, 3, S, S, dtype=torch.float64), theta=torch.zeros(B, 24, 2, 3), sel=torch.zeros(24, 6, dtype=torch.long))
    bhw = None if op == 'part_gt' else (B, S, S)
    img, th, w, sel = part_ops._gt_args(op, good['iuv_img'], good['theta'], good['sel'], torch.ones(B, dtype=torch.float64), bhw)
    assert img.dtype == th.dtype == w.dtype == torch.float32 and sel.dtype == torch.int32
    assert part_ops._gt_args(op, good['iuv_img'], good['theta'], good['sel'], None, bhw)[2] is None
    for k, bad in (('iuv_img', torch.zeros(B, 4, S, S)), ('theta', torch.zeros(B, 24, 3, 2)), ('sel', torch.zeros(24, 5, dtype=torch.long))):
        a = dict(good, **{k: bad})
        with pytest.raises(ValueError, match='^%s: bad shapes' % op):
            part_ops._gt_args(op, a['iuv_img'], a['theta'], a['sel'], None, bhw)
    if bhw is not None:
        with pytest.raises(ValueError, match='^%s: bad shapes' % op):
            part_ops._gt_args(op, torch.zeros(B, 3, S, S + 1), good['theta'], good['sel'], None, bhw)


def test_cpu_tensors_are_refused_before_the_library_is_loaded(monkeypatch, tmp_path):
    """Every glue op raises the GPU-only error for a CPU tensor -- also where the built library is missing (DANET_LIB pointing at no
    file): the check comes before the library load, which would raise 'libdanet_hip.so is missing' instead."""
    from danet_densepose2smpl_amd import _lib, iuv_ops, part_ops, loss_ops
    missing = str(tmp_path / 'no_such_libdanet_hip.so')
    monkeypatch.setenv('DANET_LIB', missing)
    monkeypatch.setattr(_lib, 'LIB_PATH', missing)
    monkeypatch.setattr(_lib, '_lib', None)
    with pytest.raises(RuntimeError, match='libdanet_hip.so is missing'):
        _lib.lib()
    heads = [torch.zeros(B, n, S, S) for n, _ in WIDTHS]
    pred = torch.zeros(B, 504, S, S)
    img, theta, sel = torch.zeros(B, 3, S, S), torch.zeros(B, 24, 2, 3), torch.zeros(24, 6, dtype=torch.long)
    scales = ((1., 0.),) * 3
    calls = [lambda: iuv_ops.iuv_global(*heads),
             lambda: iuv_ops.softargmax(torch.zeros(B, 24, S, S)),
             lambda: iuv_ops.dp_point_losses(*heads, {}),
             lambda: part_ops.part_clean(pred),
             lambda: part_ops.part_losses(pred, img, theta, None, sel, True),
             lambda: part_ops.part_joint(pred, None, img, theta, None, sel, True, scales),
             lambda: part_ops.part_gt(img, theta, sel),
             lambda: loss_ops.smpl_losses(torch.zeros(B, 229), [], [], None, None, None, None, None, None, None, None, None, 5000., 224., 0.25, 1., {})]
    for k, call in enumerate(calls):
        with pytest.raises(RuntimeError, match='GPU only.*no CPU path'):
            call()
    with pytest.raises(RuntimeError, match=r'GPU only \(part_joint: got a cpu tensor\); there is no CPU path'):
        calls[5]()
