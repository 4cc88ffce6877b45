"""TEST INFRASTRUCTURE ONLY: one fused clip + AdamW step over a flat arena, restated in plain fp64 torch.

Takes what ``clg_vqa_amd.ops.adamw`` takes and returns what the kernel leaves in ``p, m, v`` plus the scale it applied to
the gradient.  The semantics are those of ``adamw_kernel`` (csrc/elementwise.hip) and of oracle/adamw_oracle.py:

* ``sumsq`` given: ``coef = min(1, max_norm / (sqrt(sumsq) * post + 1e-6))`` with torch.clamp's treatment of NaN (a NaN
  norm gives a NaN coefficient), and the gradient is scaled by ``coef * post``; ``grad_scale`` is then ignored;
* ``m = b1 m + (1 - b1) g``, ``v = b2 v + (1 - b2) g^2``, ``p -= step_size * m / (sqrt(v) + eps)`` with
  ``step_size = lr * lr_mult`` times ``sqrt(1 - b2^t) / (1 - b1^t)`` when ``correct_bias``; ``t`` is the segment's own
  count when ``seg_step`` is given, else ``step``;
* then the decoupled decay ``p -= lr * lr_mult * wd * p``;
* a negative ``seg_lr`` marks a segment without a gradient: nothing of it changes;
* ``row_flags``: rows of the flagged table whose flag is 0 hold ``g = m = v = 0`` and only decay.

tests/test_adamw_ref_host.py pins this function to oracle.adamw_oracle.ReferenceAdamW on the CPU before the GPU tests
use it to judge the kernel."""
import math

import torch


def clip_scale(sumsq, max_norm, post):
    """The scale the kernel applies to the summed gradient: clip coefficient of the averaged gradient times 1/world."""
    norm = torch.sqrt(torch.as_tensor(sumsq, dtype=torch.float64).reshape(())) * post
    coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    return coef * post


def bias_correction(b1, b2, t, correct_bias=True):
    return math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t) if correct_bias else 1.0


def adamw_step(p, g, m, v, seg_end, seg_lr, seg_wd, b1, b2, eps, step, correct_bias, lr_mult, grad_scale=1.0, sumsq=None,
               max_norm=0.0, post=1.0, seg_step=None, row_flags=None, flag_begin=0, flag_rows=0, flag_row_len=0):
    """p, g, m, v: flat tensors (any float dtype, any device; computed in fp64 on the CPU); seg_*: sequences or tensors.
    Returns (p, m, v, gs): new fp64 CPU tensors and the applied gradient scale (fp64 scalar tensor)."""
    p, g, m, v = (t.detach().double().cpu().clone() for t in (p, g, m, v))
    ends = [int(e) for e in torch.as_tensor(seg_end).tolist()]
    lrs = [float(x) for x in torch.as_tensor(seg_lr).double().tolist()]
    wds = [float(x) for x in torch.as_tensor(seg_wd).double().tolist()]
    steps = None if seg_step is None else [int(s) for s in torch.as_tensor(seg_step).tolist()]
    gs = clip_scale(sumsq, max_norm, post) if sumsq is not None else torch.tensor(float(grad_scale), dtype=torch.float64)
    fl_end = flag_begin + flag_rows * flag_row_len
    begin = 0
    for i, end in enumerate(ends):
        lo, begin = begin, end
        if lrs[i] < 0.0:
            continue
        lr = lrs[i] * lr_mult
        t = step if steps is None else max(steps[i], 1)
        step_size = lr * bias_correction(b1, b2, t, correct_bias)
        sl = slice(lo, end)
        grad = g[sl] * gs
        mm = b1 * m[sl] + (1.0 - b1) * grad
        vv = b2 * v[sl] + (1.0 - b2) * grad * grad
        pp = p[sl] - step_size * (mm / (vv.sqrt() + eps))
        if wds[i] > 0.0:
            pp = pp - lr * wds[i] * pp
        if row_flags is not None and lo <= flag_begin < end:
            # untouched rows of the table: no moments, decay only
            assert lo == flag_begin and fl_end <= end, "the flagged table starts its segment"
            keep = torch.ones(end - lo, dtype=torch.bool)
            keep[:fl_end - lo] = torch.as_tensor(row_flags).cpu().bool().repeat_interleave(flag_row_len)
            decayed = p[sl] - lr * wds[i] * p[sl] if wds[i] > 0.0 else p[sl]
            pp, mm, vv = torch.where(keep, pp, decayed), torch.where(keep, mm, m[sl]), torch.where(keep, vv, v[sl])
        p[sl], m[sl], v[sl] = pp, mm, vv
    return p, m, v, gs
