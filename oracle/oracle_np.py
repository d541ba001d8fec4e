"""CPU oracle (numpy) for the fake-quantization hot path -- TEST INFRASTRUCTURE ONLY.

This file is a plain restatement of the reference's algorithm
(antspy/quantized_distillation, quantization/quant_functions.py and
quantization/help_functions.py) in numpy fp32 arithmetic, one separately rounded IEEE operation
per reference tensor op, in the reference's op order.  It exists to CHECK the HIP path; nothing
in the product (`quantized_distillation_amd/`, `quantization/`) imports it.  Only `tests/`,
`__graft_entry__.smoke()` and the `cpu_baseline` leg of `bench.py` may use it.

Parity pin: every function here is checked in tests/test_oracle_golden.py against the vectors in
tests/golden/*.npz, which were produced by running the unmodified reference
(tests/golden/gen_golden.py).  The reference has no tests or golden vectors of its own
(SURVEY.md section 4), so "the reference executed here" is the pin.

All `ref:` citations are relative to /root/reference/.
"""
import numpy as np

F32 = np.float32
TOL_DIFF_ZERO = 1e-10          # ref: quantization/quant_functions.py:40


# ----------------------------------------------------------------------------- bucket geometry
def bucket_geometry(n, bucket):
    """(num_buckets, row_length, padded_length) of the bucket view of an n-element tensor.

    ref: quantization/help_functions.py:67-94 -- n < bucket: one short row of n elements;
    n % bucket == 0: n/bucket full rows; otherwise one extra row padded with copies of the
    last element.  bucket None: a single row holding the whole tensor (1-D in the reference).
    """
    if bucket is None:
        return 1, n, n
    mult, rest = divmod(n, bucket)
    if mult == 0:
        return 1, n, n
    if rest == 0:
        return mult, bucket, n
    return mult + 1, bucket, (mult + 1) * bucket


def bucketize(v, bucket):
    """ref: help_functions.py:67-94 (fill_values='last').  v: 1-D fp32.  Returns 2-D rows
    (or the 1-D vector when bucket is None, as quant_functions.py:79-80 does)."""
    n = v.size
    if bucket is None:
        return v
    nb, row, padded = bucket_geometry(n, bucket)
    if padded != n:
        v = np.concatenate([v, np.full(padded - n, v[-1], dtype=F32)])
    return v.reshape(nb, row)


# ----------------------------------------------------------------------------- scaling
def scale_down(x, bucket=None, max_element=False, subtract_mean=False, mean=None):
    """Linear scaling to [0,1].  ref: quant_functions.py:56-107,129.

    Returns dict(u, alpha, beta, imin, imax, mean, n, shape).  `u` has the bucket layout
    (nb, row) -- or (n,) when bucket is None -- INCLUDING the padding of a ragged last bucket.
    `mean` overrides the fp32 mean (torch's summation order is not reproducible in numpy;
    tests pass the value the implementation under test reports).
    """
    x = np.asarray(x, dtype=F32)
    shape = x.shape
    v = x.reshape(-1).copy()
    n = v.size
    if subtract_mean:                                             # :66-68
        m = F32(np.mean(v, dtype=np.float64)) if mean is None else F32(mean)
        v = (v - m).astype(F32)
    else:
        m = F32(0.0)                                              # :70
    if max_element is not False:                                  # :72-74
        me = F32(max_element)
        v = np.where(v > me, me, v)
        v = np.where(v < -me, -me, v).astype(F32)
    t = bucketize(v, bucket)                                      # :78-81
    axis = 0 if bucket is None else 1
    mn = t.min(axis=axis, keepdims=True)                          # :85-90
    mx = t.max(axis=axis, keepdims=True)
    imin = t.argmin(axis=axis).reshape(mn.shape).astype(np.int64)  # first occurrence, like torch
    imax = t.argmax(axis=axis).reshape(mx.shape).astype(np.int64)
    alpha = (mx - mn).astype(F32)                                 # :91
    beta = mn.astype(F32)                                         # :92
    alpha = np.where(alpha < F32(TOL_DIFF_ZERO), F32(1.0), alpha).astype(F32)   # :95-99
    u = ((t - beta).astype(F32) / alpha).astype(F32)              # :106-107 (sub, then true div)
    return dict(u=u, alpha=alpha, beta=beta, imin=imin, imax=imax, mean=m, n=n, shape=shape)


def inv_scale_down(u, alpha, beta, mean, n, shape):
    """ref: quant_functions.py:131-152: mul, add (two roundings), add mean, strip padding."""
    y = (u * alpha).astype(F32)                                   # :142
    y = (y + beta).astype(F32)                                    # :143
    y = (y + F32(mean)).astype(F32)                               # :148
    return y.reshape(-1)[:n].reshape(shape)                       # :149-150


# ----------------------------------------------------------------------------- uniform
def uniform_quantize(x, s, bucket=None, max_element=False, subtract_mean=False, mean=None):
    """Deterministic k-level quantize-dequantize.  ref: quant_functions.py:155-194 (:189-191).

    Returns dict(q, lev, alpha, beta, imin, imax, mean, u).  `lev` = rint(u*(s-1)) as int32 in
    the bucket layout (padding included) -- the integer path that must match bit-exactly.
    """
    sd = scale_down(x, bucket, max_element, subtract_mean, mean)
    sm1 = F32(s - 1)                                              # :172
    t = (sd['u'] * sm1).astype(F32)                               # :189
    r = np.rint(t).astype(F32)                                    # :190 round half to even
    w = (r / sm1).astype(F32)                                     # :191
    q = inv_scale_down(w, sd['alpha'], sd['beta'], sd['mean'], sd['n'], sd['shape'])   # :193
    out = dict(sd)
    # NaN: level 0, what both libraries store; s = 2^31 - 1: s - 1 rounds to 2^31 in fp32, past int32 -- saturated
    out.update(q=q, lev=np.minimum(np.where(np.isnan(r), F32(0.0), r).astype(np.float64), 2147483647.0).astype(np.int32))
    return out


def uniform_quantize_stochastic(x, s, rand, bucket=None, max_element=False, subtract_mean=False, mean=None):
    """Stochastic-rounding variant given the uniform [0,1) draws `rand` (bucket layout).
    ref: quant_functions.py:174-187.  `rand <= prob` (:187): an element exactly on a level (prob == 0) moves one level up
    when its draw is 0.0 -- the bucket's maximum to level s, one past the top, and q follows.  `lev` is the level INDEX both
    libraries store in their optional uint8 output (include/qd_hip.h): floor + increment, saturated at s - 1, NaN as 0."""
    sd = scale_down(x, bucket, max_element, subtract_mean, mean)
    sm1 = F32(s - 1)
    prob = (sm1 * sd['u']).astype(F32)                            # :179
    t = (sd['u'] * sm1).astype(F32)                               # :180
    fl = np.floor(t).astype(F32)                                  # :181
    prob = (prob - fl).astype(F32)                                # :182
    w = (fl / sm1).astype(F32)                                    # :183
    up = np.asarray(rand, dtype=F32).reshape(w.shape) <= prob
    inc = (up.astype(F32) * F32(1.0) / sm1).astype(F32)
    w = (w + inc).astype(F32)                                     # :187
    q = inv_scale_down(w, sd['alpha'], sd['beta'], sd['mean'], sd['n'], sd['shape'])
    lev = np.minimum(fl + up.astype(F32), sm1)                    # (NaN stays NaN through np.minimum)
    out = dict(sd)
    out.update(q=q, lev=np.minimum(np.where(np.isnan(lev), F32(0.0), lev).astype(np.float64), 2147483647.0).astype(np.int32), up=up)
    return out


def philox4x32(counter, key, rounds):
    """Philox4x32 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with `rounds` rounds:
    counter = four 32-bit words, key = two 32-bit words (scalars or arrays that broadcast against each other).  Returns the four output words as
    uint64 arrays.  A round multiplies c0 by M0 and c2 by M1 and returns (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key
    is bumped by the Weyl constants AFTER each round (so the first round sees the key itself).  At 10 rounds this is
    Random123's philox4x32_10, pinned by its published known-answer vectors in tests/test_stochastic_host.py."""
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.atleast_1d(np.asarray(c, dtype=np.uint64)) & mask for c in counter])
    k0, k1 = (np.asarray(k, dtype=np.uint64) & mask for k in key)   # scalars, or arrays that broadcast against the counter
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2                                   # 32 x 32 -> 64-bit products
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & mask, p1 >> np.uint64(32), p1 & mask
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


def philox4x32_7_words(seed, n, first=0):
    """The 32-bit word behind the draw of every element index first..first + n - 1 (first % 4 == 0): Philox4x32 with 7
    rounds, counter = (element >> 2 as two words, 0x51ed270b, 0x2545f491), key = the 64-bit seed, word = element & 3."""
    assert first % 4 == 0
    blocks = np.arange(first // 4, first // 4 + (n + 3) // 4, dtype=np.uint64)
    words = philox4x32((blocks & np.uint64(0xFFFFFFFF), blocks >> np.uint64(32), 0x51ed270b, 0x2545f491),
                       (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), 7)
    return np.stack(words, axis=1).reshape(-1)[:n]


def philox4x32_7_uniform(seed, n):
    """The uniform [0,1) draw of every element index 0..n-1 under the in-kernel generator of the HIP path
    (quantized_distillation_amd/csrc/qd_common.h: philox_uniform4) -- Philox4x32 with 7 rounds, counter =
    (element >> 2, 0x51ed270b, 0x2545f491), key = the 64-bit seed, component = element & 3, and the draw is the word's
    TOP 24 bits times 2^-24: a multiple of 2^-24 in [0, 1 - 2^-24], exactly 0.0 once in 2^24 draws.
    This restates OUR generator (the reference draws torch.rand on the host, quant_functions.py:185-186, which
    no device generator can reproduce); it lets the stochastic branch be checked bit for bit on every kernel
    path instead of only statistically."""
    words = philox4x32_7_words(seed, n)
    return ((words >> np.uint64(8)).astype(np.float32) * F32(1.0 / 16777216.0)).astype(F32)


# ----------------------------------------------------------------------------- non-uniform
def assign_distance(u, pts):
    """Nearest sorted point, ties to the UPPER point.  ref: quant_functions.py:267-273."""
    pts = np.asarray(pts, dtype=F32)
    flat = u.reshape(-1)
    i = np.searchsorted(pts, flat, side='left').clip(max=pts.size - 1)            # :267-268
    lower = (i > 0) & (np.fabs(flat - pts[np.maximum(i - 1, 0)]) < np.fabs(flat - pts[i]))   # :269-272
    return (i - lower).astype(np.int64).reshape(u.shape)                           # :273


def midpoints(pts):
    """ref: quant_functions.py:533 -- k[:-1] + diff(k)/2 in fp32."""
    pts = np.asarray(pts, dtype=F32)
    return (pts[:-1] + (np.diff(pts) / F32(2.0)).astype(F32)).astype(F32)


def assign_midpoint(u, pts):
    """Index = #{midpoints <= u}: what SearchSorted.query computes through the sorted copy.
    ref: quant_functions.py:531-573 (searchsorted-left of the midpoints INTO the sorted tensor,
    :534, means element e gets index j iff exactly j midpoints are <= e)."""
    m = midpoints(pts)
    return np.searchsorted(m, u.reshape(-1), side='right').astype(np.int64).reshape(u.shape)


def nonuniform_quantize(x, pts, bucket=None, mode='distance', max_element=False, subtract_mean=False, mean=None):
    """ref: quant_functions.py:196-290.  mode 'distance' = plain path (:267-273), 'midpoint' =
    pre-processed path (:275 -> SearchSorted.query).  Returns dict(q, idx, alpha, beta, ...);
    idx is int64 with the ORIGINAL shape (:288-289)."""
    pts = np.asarray(pts, dtype=F32)
    sd = scale_down(x, bucket, max_element, subtract_mean, mean)
    idx_full = assign_distance(sd['u'], pts) if mode == 'distance' else assign_midpoint(sd['u'], pts)
    w = pts[idx_full]                                                               # :278
    q = inv_scale_down(w, sd['alpha'], sd['beta'], sd['mean'], sd['n'], sd['shape'])   # :286-287
    idx = idx_full.reshape(-1)[:sd['n']].reshape(sd['shape'])
    out = dict(sd)
    out.update(q=q, idx=idx)
    return out


def point_grad(g, idx, alpha, bucket, k, dtype=np.float64):
    """gradPoint[j] = sum_{i: idx_i == j} g_i * alpha_bucket(i).  ref: quant_functions.py:493-503.
    The product g*alpha is one fp32 multiply (:495); the per-bin sum is accumulated in `dtype`
    (float64 by default = the exact-ish value both torch's fp32 sum and the HIP reduction are
    compared against, with a tolerance relative to sum|g*alpha|)."""
    g = np.asarray(g, dtype=F32).reshape(-1)
    idx = np.asarray(idx).reshape(-1)
    n = g.size
    if bucket is None:
        a = np.broadcast_to(np.asarray(alpha, dtype=F32).reshape(-1)[:1], (n,))
    else:
        nb, row, _ = bucket_geometry(n, bucket)
        a = np.repeat(np.asarray(alpha, dtype=F32).reshape(-1), row)[:n]
    mg = (g * a).astype(F32)
    out = np.zeros(k, dtype=dtype)
    np.add.at(out, idx, mg.astype(dtype))
    absum = np.zeros(k, dtype=np.float64)
    np.add.at(absum, idx, np.abs(mg).astype(np.float64))
    return out, absum


# ----------------------------------------------------------------------------- STE variants
def ste_complicated_backward(x, g, s, bucket, tie_mode='reference'):
    """'complicated' straight-through backward.  ref: quant_functions.py:319-406 with the two
    shape fixes of SURVEY.md 8c (the shipped code raises for > 1 bucket).

    Closed form: per bucket S_b = sum_i g_i*(qs_i - u_i) over the real (non
    padded) elements, out = g, out[jmax_b] += S_b, out[jmin_b] -= S_b.
    Reference-faithful details reproduced here:
      * :350 re-runs scale_down on the QUANTIZED tensor, so alpha/beta/jmin/jmax are those of q
        (jmax = first element at the top level; tie_mode 'reference'), and qs = (q-beta_q)/alpha_q;
      * u_i = (x_i - beta_q)/alpha_q (:400) uses the same re-derived alpha/beta.
      * the sum is what torch.mm of the sparse +-1 matrix does: fp32 accumulate; we accumulate in
        float64 and compare with tolerance.
    tie_mode 'true_arg' uses argmax/argmin of x instead.
    """
    x = np.asarray(x, dtype=F32)
    g = np.asarray(g, dtype=F32)
    shape = x.shape
    n = x.size
    uq = uniform_quantize(x, s, bucket)
    q = uq['q']
    sdq = scale_down(q, bucket)                       # :350 (overwrites alpha, beta, idx)
    nb, row, padded = bucket_geometry(n, bucket)
    qs = sdq['u'].reshape(-1)[:n]
    alpha = np.repeat(sdq['alpha'].reshape(-1), row)[:n]
    beta = np.repeat(sdq['beta'].reshape(-1), row)[:n]
    u = ((x.reshape(-1) - beta).astype(F32) / alpha).astype(F32)       # :400 (tensor-beta)/alpha
    term = (g.reshape(-1) * (qs - u).astype(F32)).astype(F32)
    if tie_mode == 'reference':
        jmax, jmin = sdq['imax'].reshape(-1), sdq['imin'].reshape(-1)
    else:
        sdx = scale_down(x, bucket)
        jmax, jmin = sdx['imax'].reshape(-1), sdx['imin'].reshape(-1)
    out = g.reshape(-1).astype(np.float64).copy()
    for b in range(nb):
        lo, hi = b * row, min((b + 1) * row, n)
        sb = term[lo:hi].astype(np.float64).sum()
        # the reference adds grad_alpha^T . term: column jmax gets +sum over rows i of the bucket
        # whose (expanded, truncated to n) idx points at it
        out[lo + jmax[b]] += sb
        out[lo + jmin[b]] -= sb
    return out.astype(F32).reshape(shape)


def ste_bucket_terms(x, g, s, bucket, tie_mode='reference'):
    """The pieces of the 'complicated' STE backward per bucket, for tolerance checks of the bucket SUM (the only
    floating-point reduction of that function): terms t_i = g_i * (qs_i - u_i) exactly as the reference rounds them in
    fp32 (quant_functions.py:350, :400), then
        sb[b]        = float64 sum of the bucket's terms,
        abs_terms[b] = float64 sum of |t_i|  (what a summation error is measured against),
        jmax[b], jmin[b] = the two positions (relative to the bucket start) the sum is added to / subtracted from.
    Vectorised (no Python loop over buckets)."""
    x = np.asarray(x, dtype=F32).reshape(-1)
    g = np.asarray(g, dtype=F32).reshape(-1)
    n = x.size
    q = uniform_quantize(x, s, bucket)['q'].reshape(-1)
    sdq = scale_down(q, bucket)
    nb, row, padded = bucket_geometry(n, bucket)
    qs = sdq['u'].reshape(-1)[:n]
    alpha = np.repeat(sdq['alpha'].reshape(-1), row)[:n]
    beta = np.repeat(sdq['beta'].reshape(-1), row)[:n]
    u = ((x - beta).astype(F32) / alpha).astype(F32)
    term = (g * (qs - u).astype(F32)).astype(F32).astype(np.float64)
    starts = np.arange(nb, dtype=np.int64) * row
    sb = np.add.reduceat(term, starts)
    abs_terms = np.add.reduceat(np.abs(term), starts)
    if tie_mode == 'reference':
        jmax, jmin = sdq['imax'].reshape(-1), sdq['imin'].reshape(-1)
    else:
        sdx = scale_down(x, bucket)
        jmax, jmin = sdx['imax'].reshape(-1), sdx['imin'].reshape(-1)
    return {'sb': sb, 'abs_terms': abs_terms, 'jmax': np.asarray(jmax, np.int64), 'jmin': np.asarray(jmin, np.int64),
            'row': row, 'nb': nb}


def truncated_ste_mask(w, grad):
    """'truncated' STE: grad[|w| > 1] = 0.  ref: cnn_models/conv_forward_model.py:263-264."""
    w = np.asarray(w, dtype=F32)
    out = np.asarray(grad, dtype=F32).copy()
    out[np.abs(w) > F32(1.0)] = F32(0.0)
    return out


# ----------------------------------------------------------------------------- setup helpers
def init_points_percentile(x, bucket, k, max_element=False, subtract_mean=False):
    """ref: help_functions.py:140-154 -- np.percentile (linear interpolation, float64) of the
    scaled tensor without padding, cast back to fp32."""
    sd = scale_down(x, bucket, max_element, subtract_mean)
    flat = sd['u'].reshape(-1)[:sd['n']]
    return np.percentile(flat, np.linspace(0, 100, num=k)).astype(F32)


# ----------------------------------------------------------------------------- absmax / absnorm
# PARITY UNPINNED: the reference's code for these scaling types (quant_functions.py:109-127,144-146)
# raises on every torch version, so there is no reference OUTPUT to pin against.  This restates the math
# those lines evidently intend, one fp32 operation per torch op of the repaired lines, with the rules of
# include/qd_hip.h (NaN / inf section, abs paragraph); oracle/torch_port.py states the same with torch's
# own CPU ops and tests/test_abs_cases_host.py holds the two together.
def torch_sign(t):
    """torch.sign: 0 for +-0 and for a NaN of either sign bit and any payload (np.sign gives NaN), +-1 otherwise."""
    t = np.asarray(t, dtype=F32)
    return np.where(t > 0, F32(1.0), np.where(t < 0, F32(-1.0), F32(0.0))).astype(F32)


def abs_norm(m, kind):
    """Per-row norm of the magnitudes m (2-D, fp32) before the 1e-10 guard: max (a NaN propagates, as torch.max), or
    sqrt(sum m^2) with fp32 squares (they overflow to inf and underflow to 0 as torch's do), the sum of those squares taken
    in float64 and rounded to fp32 once, fp32 square root."""
    if kind == 'absmax':
        return m.max(axis=1, keepdims=True).astype(F32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        sq = (m * m).astype(F32)
        return np.sqrt(sq.astype(np.float64).sum(axis=1, keepdims=True).astype(F32)).astype(F32)


def scale_down_abs(x, bucket=None, kind='absmax', norm=None, max_element=False, subtract_mean=False, mean=None):
    """sign, u = |v| / norm_b with v = x after mean subtraction and clamping (as scale_down) and norm_b = max|v| ('absmax')
    or sqrt(sum v^2) ('absnorm') per bucket, norm < 1e-10 -> 1 (a NaN norm stays).  `norm` overrides the per-bucket norms
    (the summation order of the L2 norm is implementation specific), `mean` the fp32 mean.  Returns dict(u, sign, norm, mean,
    n, shape); u and sign in the padded bucket layout."""
    x = np.asarray(x, dtype=F32)
    v = x.reshape(-1).copy()
    n = v.size
    with np.errstate(invalid='ignore'):
        if subtract_mean:
            mu = F32(np.mean(v, dtype=np.float64)) if mean is None else F32(mean)
            v = (v - mu).astype(F32)
        else:
            mu = F32(0.0)
        if max_element is not False:
            me = F32(max_element)
            v = np.where(v > me, me, v)
            v = np.where(v < -me, -me, v).astype(F32)
        t = bucketize(v, bucket)
        t2 = t.reshape(1, -1) if bucket is None else t
        sign = torch_sign(t2)
        m = np.abs(t2)
        if norm is None:
            nrm = abs_norm(m, kind)
            nrm = np.where(nrm < F32(TOL_DIFF_ZERO), F32(1.0), nrm).astype(F32)
        else:
            nrm = np.asarray(norm, dtype=F32).reshape(-1, 1)
        u = (m / nrm).astype(F32)
    return dict(u=u.reshape(t.shape), sign=sign.reshape(t.shape), norm=nrm.reshape(-1), mean=mu, n=n, shape=x.shape)


def inv_scale_down_abs(u, sign, norm, mean, n, shape):
    """y = u * norm_b * sign + mean, one rounding each, padding dropped."""
    nrm = np.asarray(norm, dtype=F32).reshape(-1, 1)
    with np.errstate(invalid='ignore', over='ignore'):
        y = (np.asarray(u, dtype=F32).reshape(nrm.size, -1) * nrm).astype(F32)
        y = (y * np.asarray(sign, dtype=F32).reshape(y.shape)).astype(F32)
        y = (y + F32(mean)).astype(F32)
    return y.reshape(-1)[:n].reshape(shape)


def uniform_quantize_abs(x, s, bucket=None, kind='absmax', norm=None, max_element=False, subtract_mean=False, mean=None):
    sd = scale_down_abs(x, bucket, kind, norm, max_element, subtract_mean, mean)
    sm1 = F32(s - 1)
    u2 = sd['u'].reshape(sd['norm'].size, -1)
    with np.errstate(invalid='ignore', over='ignore'):
        w = (np.rint((u2 * sm1).astype(F32)).astype(F32) / sm1).astype(F32)
    out = dict(sd)
    out['q'] = inv_scale_down_abs(w, sd['sign'], sd['norm'], sd['mean'], sd['n'], sd['shape'])
    return out
