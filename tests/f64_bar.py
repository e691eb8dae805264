"""What the per-kernel float64 suites (test_gpu_train_ops.py, test_gpu_infer_ops.py, test_gpu_train_h16_ops.py) share: the two kinds of seeded
data and the element-wise bars of the random cases (bar: an fp32 result; bar16: an fp32 result stored as fp16)."""
import numpy as np
import torch


def ints(rs, *shape):
    return torch.from_numpy(rs.randint(-3, 4, size=shape).astype(np.float32))


def normal(rs, *shape):
    return torch.from_numpy(rs.standard_normal(size=shape).astype(np.float32))


def bar(name, tag, got, ref64, ref32, slack=None, keep=None):
    """element-wise |got - ref64| <= 4 * e32 + 4 ulp (+ slack); `keep`: the elements that take part"""
    got, ref64, ref32 = got.double(), ref64.double(), ref32.double()
    e32 = float((ref32 - ref64).abs().max())
    ulp = float(np.spacing(np.float32(float(ref64.abs().max()))))
    bar = 4 * e32 + 4 * ulp
    d = (got - ref64).abs()
    if slack is not None:
        d = (d - slack).clamp_min(0.0)
    if keep is not None:
        d = d[keep]
    err = float(d.max()) if d.numel() else 0.0
    print("RATIO %-8s %-22s err %.3e  e32 %.3e  ulp %.3e  err/bar %.3f" % (name, tag, err, e32, ulp, err / bar))
    assert err <= bar, "%s of %s: error %.3e against 4 * e32 + 4 ulp = %.3e (e32 %.3e)" % (name, tag, err, bar, e32)
    return err / bar


def u16(v):
    """the spacing of fp16 numbers at |v|: 2**(floor(log2 |v|) - 10), and 2**-24 below the normal range"""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -14))             # |v| = m * 2**e, 0.5 <= m < 1
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 11).double())


def bar16(name, tag, got, ref64, ref32, slack=None, keep=None):
    """a result the kernel rounds ONCE to fp16: element-wise |got - ref64| <= u16(|ref64| + d) / 2 + d (+ slack), d = 4 * e32 + 4 ulp what `bar`
    allows the fp32 value in front of the rounding; `keep`: the elements that take part"""
    got, ref64, ref32 = got.double(), ref64.double(), ref32.double()
    e32 = float((ref32 - ref64).abs().max())
    ulp = float(np.spacing(np.float32(float(ref64.abs().max()))))
    d = 4 * e32 + 4 * ulp
    allowed = u16(ref64.abs() + d) / 2 + d
    if slack is not None:
        allowed = allowed + slack
    ratio = (got - ref64).abs() / allowed
    if keep is not None:
        ratio = ratio[keep]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print("RATIO %-8s %-26s e32 %.3e  ulp %.3e  err/bar16 %.3f" % (name, tag, e32, ulp, worst))
    assert worst <= 1.0, "%s of %s: an element is %.3f times its bar u16(|ref| + d) / 2 + d, d = %.3e (e32 %.3e)" % (name, tag, worst, d, e32)
    return worst
