"""What the duality-gap tests share (settings.check_dualgap on the batch routes; tests/test_batch_gap_rules.py on the CPU,
tests/test_gpu_lockstep_supp.py and tests/test_gpu_batch_dualgap.py on the GPU):

  * the support term and its sum in np.longdouble, the numpy stand-in of k_ls_supp (osqp-python_amd/csrc/lockstep_hip.hip) in the kernel's own summation
    order, and the judge of that kernel's partials with the bound gamma_k sum |terms|;
  * the gap of a returned (x, y) recomputed on the host in np.longdouble from the unscaled data, with its bound (n + m + r) 2^-53 S;
  * the gap test |gap| < eps_abs + eps_rel max(|obj|, |dual_obj|), x 10 on the approximate pass.
"""
import numpy as np

W = 64
LD = np.longdouble
U53 = 2.0 ** -53
FINITE = 1e30 * 1e-4          # step_rules.h upper_is_finite / lower_is_finite: a bound beyond OSQP_INFTY * MIN_SCALING is no bound
SOLVED, SOLVED_INACC, MAX_ITER = 1, 2, 7


def support_terms(l, u, y, dt=LD):
    """step_rules.h support_finite per entry: u y where y > 0 and u is finite, l y where y < 0 and l is finite, else 0"""
    l, u, y = (np.asarray(a, dt) for a in (l, u, y))
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where((y > 0) & (u < FINITE), u * y, np.where((y < 0) & (l > -FINITE), l * y, dt(0)))


# ---------------------------------------------------------------------------------------------------------------- k_ls_supp
def standin_supp(l, u, y, G, term=None):
    """k_ls_supp in float64 and in the kernel's order: wave w of workgroup g adds the terms of rows 4 g + w, + 4 G, .. in row order from 0, the four waves
    are combined ((w0 + w1) + w2) + w3 (ls_put).  l, u, y: (m, 64).  -> partials (G, 64).  term: another term function (the planted mistakes)."""
    t = (term or (lambda a, b, c: support_terms(a, b, c, np.float64)))(l, u, y)
    m = t.shape[0]
    part = np.zeros((G, W))
    for g in range(G):
        wv = []
        for w in range(4):
            s = np.zeros(W)
            for i in range(4 * g + w, m, 4 * G):
                s = s + t[i]
            wv.append(s)
        part[g] = ((wv[0] + wv[1]) + wv[2]) + wv[3]
    return part


def fold_sum(part):
    """ls_fold<false>: wave w adds the partials g = w, w + 4, .. from 0, the four results are combined in wave order.  (G, 64) -> (64,)"""
    G = part.shape[0]
    f = []
    for w in range(4):
        s = np.zeros(W)
        for g in range(w, G, 4):
            s = s + part[g]
        f.append(s)
    return ((f[0] + f[1]) + f[2]) + f[3]


def supp_roundings(m, G):
    """roundings a term can pass through on its way into a workgroup's partial, counted from k_ls_supp's order: 1 (the product), at most ceil(m / 4 G)
    (the lane's adds over its wave's rows; the first add, to 0, is exact and is counted all the same), 3 (the four waves); into the folded sum: at most
    ceil(G / 4) + 3 more (ls_fold).  -> (k of a partial, k of the folded sum)"""
    k = 1 + -(-m // (4 * G)) + 3
    return k, k + -(-G // 4) + 3


def gamma(k):
    return k * U53 / (1 - k * U53)


def judge_supp(part, l, u, y, G):
    """part (G, 64): what a candidate wrote to its slot.  Every partial and the folded sum against the np.longdouble sum of the same terms, bound
    gamma_k sum |terms| with k from supp_roundings; a term set whose sum of absolute values is 0 must give exactly 0.  -> the worst ratio to the bound;
    AssertionError above 1."""
    t = support_terms(l, u, y)
    m = t.shape[0]
    kp, kf = supp_roundings(m, G)
    worst = 0.0
    tot, tot_abs = np.zeros(W, LD), np.zeros(W, LD)
    for g in range(G):
        rows = np.concatenate([np.arange(4 * g + w, m, 4 * G) for w in range(4)]).astype(int)
        ref, mag = t[rows].sum(axis=0), np.abs(t[rows]).sum(axis=0)
        tot += ref; tot_abs += mag
        err = np.abs(np.asarray(part[g], LD) - ref)
        assert np.all(np.isfinite(np.asarray(part[g]))), ('not finite', g)
        assert np.all(err[mag == 0] == 0), ('a sum of no terms is not 0', g)
        ok = mag > 0
        if ok.any():
            worst = max(worst, float((err[ok] / (gamma(kp) * mag[ok])).max()))
    err = np.abs(np.asarray(fold_sum(np.asarray(part, np.float64)), LD) - tot)
    ok = tot_abs > 0
    if ok.any():
        worst = max(worst, float((err[ok] / (gamma(kf) * tot_abs[ok])).max()))
    assert worst <= 1.0, worst
    return worst


# ---------------------------------------------------------------------------------------------------------------- the gap of a returned point
ROUNDINGS_SCALING = 16        # r of the bound: roundings per term that the scaled space adds to the products of a plain evaluation -- x = D x~ and y = cinv E y~
                              # on the way out (1 + 2), the scaled entries c D P D and E A D (3 + 2), q~ = c D q and l~ = E l (2 + 1), the kernel's own product
                              # and FMA chain entry (2), the final times cinv and the subtraction (2): 15, taken as 16


def gap_host(P, q, A, l, u, x, y):
    """-> (gap, S) in np.longdouble from the unscaled data: gap = x'Px + q'x + sum_i support_finite(l_i, u_i, y_i)  (= obj - dual_obj with
    obj = 1/2 x'Px + q'x, dual_obj = -1/2 x'Px - supp), S = the sum of the absolute values of every term (P symmetric, given whole or as its upper
    triangle: the caller passes the whole matrix)."""
    Pc = P.tocoo()
    x, y, q = np.asarray(x, LD), np.asarray(y, LD), np.asarray(q, LD)
    tp = np.asarray(Pc.data, LD) * x[Pc.row] * x[Pc.col]
    tq = q * x
    ts = support_terms(l, u, y)
    return tp.sum() + tq.sum() + ts.sum(), np.abs(tp).sum() + np.abs(tq).sum() + np.abs(ts).sum()


def gap_bound(n, m, S):
    return (n + m + ROUNDINGS_SCALING) * U53 * float(S)


def gap_ok_values(obj, dual_obj, gap, eps_abs, eps_rel, approx=False):
    """term_rules.h term_gap_ok, the same operations in the same order (a NaN anywhere: False)"""
    f = 10.0 if approx else 1.0
    return abs(gap) < f * eps_abs + (f * eps_rel) * max(abs(obj), abs(dual_obj))


def gap_passes(obj, gap, eps_abs, eps_rel, approx=False):
    """the gap test on a record's columns 2 and 11: dual_obj = obj - gap"""
    return gap_ok_values(obj, obj - gap, gap, eps_abs, eps_rel, approx)
