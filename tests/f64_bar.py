"""What the per-kernel float64 suites (test_gpu_train_ops.py, test_gpu_infer_ops.py) share: the two kinds of seeded data and the
element-wise bar of the random cases."""
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
