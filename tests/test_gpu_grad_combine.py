"""GPU tests of wn_grad_combine (csrc/wn_train.hip): bit for bit train.combine_np -- the float32 left-to-right
sum of the rows times float32(1 / S) -- at every row count that takes another path through the kernel (1: no add; 2, 3: the
remainder loop; 8: seven adds, still the remainder loop; 9: one batch of eight loads; 64: seven batches, a remainder of
seven, and the bound of the call), at sizes around the quad (1, 3, 4, 5), a size with a tail over several blocks (1 023) and
one past 2^16 (65 537), on the vector and on the scalar path, with `out` beside the rows, offset by one float, and aliasing
row 0."""
import numpy as np
import pytest
import torch

from nsynth_wavenet_amd import train

pytestmark = pytest.mark.gpu
ROWS = [1, 2, 3, 8, 9, 64]
SIZES = [1, 3, 4, 5, 1023, 65537]
PAD = 0x7FC00123                  # a NaN pattern: whatever the kernel must not touch


def _host_rows(S, n, seed):
    rs = np.random.RandomState(seed)
    # magnitudes over twelve octaves and both signs, so that an add in another order rounds differently
    return (rs.standard_normal([S, n]) * np.exp2(rs.randint(-6, 7, [S, n]))).astype(np.float32)


@pytest.fixture(scope='module')
def cases():
    """{(S, n): (host rows, combine_np of them)}: computed once, shared, never written to"""
    out = {}
    for S in ROWS:
        for n in SIZES:
            rows = _host_rows(S, n, 1000 * S + n % 997)
            want = train.combine_np(list(rows))
            rows.setflags(write=False)
            want.setflags(write=False)
            out[S, n] = (rows, want)
    return out


def _padded(S, stride, rows, lead=0):
    """device buffer of lead + S * stride floats, NaN-patterned, with the rows at lead + j * stride; returns (buffer, view)"""
    n = rows.shape[1]
    buf = torch.full([lead + S * stride], PAD, dtype=torch.int32, device='cuda').view(torch.float32)
    view = buf[lead:].view(S, stride)[:, :n]
    view.copy_(torch.from_numpy(rows.copy()))
    return buf, view


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('S', ROWS)
def test_contiguous_rows(cases, S):
    """[S, n] as torch lays it out: the vector path where n % 4 == 0 (or S == 1), the scalar path otherwise"""
    from nsynth_wavenet_amd.engine import grad_combine
    for n in SIZES:
        rows, want = cases[S, n]
        dev = torch.from_numpy(rows.copy()).cuda()
        got = grad_combine(dev)
        assert got.shape == (n,) and got.dtype == torch.float32
        assert np.array_equal(_bits(got), want.view(np.uint32)), (S, n)
        assert np.array_equal(_bits(grad_combine(dev)), _bits(got))              # a repeated call: the same bytes
        assert np.array_equal(_bits(dev), rows.view(np.uint32))                  # the rows are read only


@pytest.mark.parametrize('S', ROWS)
@pytest.mark.parametrize('stride_extra', [4, 8, 1, 3], ids=['stride+4', 'stride+8', 'stride+1-scalar', 'stride+3-scalar'])
def test_strided_rows(cases, S, stride_extra):
    """row_stride > n; a stride that is no multiple of 4 floats forces the scalar path (for n % 4 == 0, +1 and +3 are odd)"""
    from nsynth_wavenet_amd.engine import grad_combine
    for n in SIZES:
        rows, want = cases[S, n]
        stride = (n + 3) // 4 * 4 + stride_extra
        buf, view = _padded(S, stride, rows)
        assert view.stride(0) == stride and (stride % 2 == 1) == (stride_extra in (1, 3))
        before = _bits(buf).copy()
        got = grad_combine(view)
        assert np.array_equal(_bits(got), want.view(np.uint32)), (S, n, stride)
        assert np.array_equal(_bits(buf), before)                                 # nothing between the rows was written


@pytest.mark.parametrize('S', ROWS)
def test_out_offset_by_one_float_and_rows_off_the_grid(cases, S):
    from nsynth_wavenet_amd.engine import grad_combine
    for n in SIZES:
        rows, want = cases[S, n]
        # out one float into a NaN-patterned buffer: the floats on both sides of it stay
        obuf = torch.full([n + 2], PAD, dtype=torch.int32, device='cuda').view(torch.float32)
        buf, view = _padded(S, (n + 3) // 4 * 4, rows)
        got = grad_combine(view, out=obuf[1:1 + n])
        assert got.data_ptr() == obuf.data_ptr() + 4
        ob = _bits(obuf)
        assert ob[0] == PAD and ob[-1] == PAD and np.array_equal(ob[1:-1], want.view(np.uint32)), (S, n)
        # the rows themselves one float off the grid
        buf, view = _padded(S, (n + 3) // 4 * 4, rows, lead=1)
        assert view.data_ptr() % 16 == 4
        assert np.array_equal(_bits(grad_combine(view)), want.view(np.uint32)), (S, n)


@pytest.mark.parametrize('S', ROWS)
def test_out_may_be_row_0(cases, S):
    from nsynth_wavenet_amd.engine import grad_combine
    for n in SIZES:
        rows, want = cases[S, n]
        for stride in ((n + 3) // 4 * 4, n + (1 - n % 2)):                        # the vector path, and an odd stride
            stride = max(stride, n)
            buf, view = _padded(S, stride, rows)
            got = grad_combine(view, out=view[0])
            assert got.data_ptr() == view.data_ptr()
            assert np.array_equal(_bits(view[0]), want.view(np.uint32)), (S, n, stride)
            if S > 1:
                assert np.array_equal(_bits(view[1:]), rows[1:].view(np.uint32))  # the other rows are as they were
            full = _bits(buf).reshape(S, stride)
            assert (full[:, n:] == PAD).all()


def test_refusals():
    from nsynth_wavenet_amd.engine import grad_combine
    x = torch.zeros(4, 8, device='cuda')
    with pytest.raises(ValueError, match='65 rows; the combine takes 1 to 64'):
        grad_combine(torch.zeros(65, 4, device='cuda'))
    with pytest.raises(ValueError, match=r'must be a \[S, n\] float32 device tensor'):
        grad_combine(x.double())
    with pytest.raises(ValueError, match='unit inner stride'):
        grad_combine(x[:, ::2])
    with pytest.raises(ValueError, match='out must be a flat float32 tensor of 8 values'):
        grad_combine(x, out=torch.zeros(7, device='cuda'))
    with pytest.raises(ValueError, match='out overlaps rows'):
        grad_combine(x, out=x[1])
    with pytest.raises(ValueError, match='out overlaps rows'):
        grad_combine(x.view(-1)[:24].view(3, 8)[:, :6], out=x.view(-1)[2:8])
