"""CPU restatement of the reference's uniformQuantization as the SAME SEQUENCE OF TORCH CPU OPS
(clone, cat, min, max, sub_, div_, mul_, round_, div_, mul_, add_, add_) -- TEST/BENCH
INFRASTRUCTURE ONLY.

The reference's CPU path is exactly this chain of multi-threaded torch ops
(quantization/quant_functions.py:155-194 with :56-107 and :131-152, help_functions.py:67-94).
/root/reference does not exist on the GPU box, so bench.py times this port there as
`cpu_baseline_torch_ops` (next to the scalar C port with OpenMP).  Checked bit-for-bit against
the golden vectors in tests/test_oracle_golden.py::test_torch_port.  Never imported by the
product."""
import torch


def uniform_quantize_torch_ops(x, s, bucket=None):
    t = x.clone()                                               # quant_functions.py:162-163
    shape, n = t.size(), t.numel()
    flat = t.view(-1)
    if bucket is not None:                                      # help_functions.py:67-94
        full, rest = divmod(n, bucket)
        if full != 0 and rest != 0:
            flat = torch.cat([flat, torch.ones(bucket - rest) * flat[-1]])
        flat = flat.view(1, n) if full == 0 else flat.view(-1, bucket)
        dim = 1
    else:
        dim = 0
    lo, _ = flat.min(dim=dim, keepdim=True)                     # :85-90
    hi, _ = flat.max(dim=dim, keepdim=True)
    alpha = hi - lo
    alpha[alpha < 1e-10] = 1                                    # :95-99
    flat.sub_(lo.expand_as(flat))                               # :106
    flat.div_(alpha.expand_as(flat))                            # :107
    flat.mul_(s - 1)                                            # :189
    flat.round_()                                               # :190
    flat.div_(s - 1)                                            # :191
    flat.mul_(alpha.expand_as(flat))                            # :142
    flat.add_(lo.expand_as(flat))                               # :143
    flat.add_(0)                                                # :148
    return flat.view(-1)[0:n].view(shape), alpha, lo


def abs_scaling_torch_ops(x, kind, s, bucket=None, norm=None, mean=None, max_element=False):
    """The 'absmax' / 'absnorm' scaling types as a sequence of torch CPU ops on fp32 tensors.  The reference's own lines
    (quant_functions.py:109-127, 144-146) raise on every torch version, so this is no port of running code: it is the evident
    repair of those lines -- torch.sign, abs, max(dim) or (m * m).sum(dim).sqrt(), the 1e-10 guard, true division, and for the
    way back mul, mul, add -- stated independently of oracle/oracle_np.py, which tests/test_abs_cases_host.py holds to it.
    x: 1-D fp32 tensor; mean: the value to subtract (None: subtract_mean off); norm: per-bucket norms to use instead of the
    computed ones.  Returns dict(sign, u, norm, back, q) as tensors, sign and u in the padded bucket layout."""
    flat = x.clone().view(-1)
    n = flat.numel()
    if mean is not None:                                        # :66-68
        flat = flat - mean
    if max_element is not False:                                # :72-74
        flat[flat > max_element] = max_element
        flat[flat < -max_element] = -max_element
    if bucket is not None:                                      # help_functions.py:67-94
        full, rest = divmod(n, bucket)
        if full != 0 and rest != 0:
            flat = torch.cat([flat, torch.ones(bucket - rest) * flat[-1]])
        flat = flat.view(1, n) if full == 0 else flat.view(-1, bucket)
    else:
        flat = flat.view(1, n)
    sign = torch.sign(flat)                                     # :111
    m = flat.abs()                                              # :112
    if norm is None:
        if kind == 'absmax':
            norm = m.max(dim=1, keepdim=True)[0]                # :114-120 as intended
        else:
            norm = (m * m).sum(dim=1, keepdim=True).sqrt()
        norm[norm < 1e-10] = 1                                  # :122-125
    else:
        norm = torch.as_tensor(norm, dtype=torch.float32).view(-1, 1)
    u = m / norm                                                # :127
    add = 0 if mean is None else mean

    def back(w):                                                # :144-148
        return (w * norm * sign + add).view(-1)[0:n]
    q = back(torch.round(u * (s - 1)) / (s - 1))                # :189-191
    return dict(sign=sign, u=u, norm=norm.view(-1), back=back(u), q=q)
