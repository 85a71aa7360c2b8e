"""fp64 numpy restatements of the distribution metrics (FID, MMD, KID) the tests compare the HIP path against.  Nothing here comes from
the reference: the formulas are the ones in the docstring of medical_image_generation_amd/metrics.py.

Every function returns (value, scale): `scale` is the magnitude the tests' absolute tolerance is relative to (FID: |mu_x - mu_y|^2 +
tr S_x + tr S_y; MMD and KID: the sum of the absolute values of the three terms)."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _fid_parts(x, y):
    x, y = _f64(x), _f64(y)
    n, m = x.shape[0], y.shape[0]
    mx, my = x.mean(0), y.mean(0)
    xc, yc = x - mx, y - my
    d2 = float(((mx - my) ** 2).sum())
    trx, try_ = float((xc * xc).sum()) / (n - 1), float((yc * yc).sum()) / (m - 1)
    return xc, yc, d2, trx, try_


def fid_gram(x, y):
    """FID through the identity tr sqrtm(S_x S_y) = || Xc Yc^T ||_* / sqrt((n-1)(m-1)), singular values from numpy.linalg.svd."""
    xc, yc, d2, trx, try_ = _fid_parts(x, y)
    n, m = xc.shape[0], yc.shape[0]
    nuc = float(np.linalg.svd(xc @ yc.T, compute_uv=False).sum())
    return d2 + trx + try_ - 2.0 * nuc / np.sqrt((n - 1.0) * (m - 1.0)), d2 + trx + try_


def fid_upstream(x, y, eps=1e-6):
    """The upstream form: numpy cov, scipy.linalg.sqrtm of the product, the eps * I retry when the root is not finite, real part."""
    from scipy import linalg
    x, y = _f64(x), _f64(y)
    mx, my = x.mean(0), y.mean(0)
    sx, sy = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    covmean = linalg.sqrtm(sx @ sy)
    if not np.isfinite(covmean).all():
        off = np.eye(sx.shape[0]) * eps
        covmean = linalg.sqrtm((sx + off) @ (sy + off))
    covmean = np.real(covmean)
    d2 = float(((mx - my) ** 2).sum())
    return d2 + np.trace(sx) + np.trace(sy) - 2.0 * np.trace(covmean), d2 + np.trace(sx) + np.trace(sy)


def _three_terms(kyy, kpp, kpy):
    m, n = kyy.shape[0], kpp.shape[0]
    a = (kyy.sum() - np.trace(kyy)) / (m * (m - 1.0))
    b = (kpp.sum() - np.trace(kpp)) / (n * (n - 1.0))
    c = 2.0 * kpy.sum() / (m * n)
    return float(a + b - c), float(abs(a) + abs(b) + abs(c))


def mmd(y, y_pred):
    """Upstream's linear-kernel estimator on the flattened batches: three Gram matrices of the raw rows."""
    y, p = _f64(y).reshape(len(y), -1), _f64(y_pred).reshape(len(y_pred), -1)
    return _three_terms(y @ y.T, p @ p.T, p @ y.T)


def kid(x, y, degree=3, gamma=None, coef0=1.0):
    """Unbiased MMD^2 with k(a, b) = (gamma a.b + coef0)^degree over the whole sets."""
    x, y = _f64(x), _f64(y)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma

    def k(a, b):
        return (gamma * (a @ b.T) + coef0) ** degree

    return _three_terms(k(x, x), k(y, y), k(x, y))


def kid_brute(x, y, degree=3, gamma=None, coef0=1.0):
    """The same sum as three explicit double loops."""
    x, y = _f64(x), _f64(y)
    n, m = len(x), len(y)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma

    def k(a, b):
        return (gamma * sum(float(u) * float(v) for u, v in zip(a, b)) + coef0) ** degree

    sxx = sum(k(x[i], x[j]) for i in range(n) for j in range(n) if i != j)
    syy = sum(k(y[i], y[j]) for i in range(m) for j in range(m) if i != j)
    sxy = sum(k(x[i], y[j]) for i in range(n) for j in range(m))
    return sxx / (n * (n - 1)) + syy / (m * (m - 1)) - 2 * sxy / (n * m)


def jacobi_sweeps(a, max_sweeps=60):
    """The device's one-sided Jacobi rule on the host (round-robin pairs, rotate when |gamma| > 2^-50 sqrt(alpha beta) and alpha beta >
    0): (singular values, sweeps run, the last one without a rotation).  Used to pin the sweep cap, not as a reference value."""
    a = _f64(a).copy()
    if a.shape[1] > a.shape[0]:
        a = a.T.copy()
    c = a.shape[1]
    if c & 1:
        a = np.concatenate([a, np.zeros((a.shape[0], 1))], 1)
    cp, N = a.shape[1], a.shape[1] - 1
    for sweep in range(1, max_sweeps + 1):
        rotations = 0
        for rd in range(N):
            i = np.arange(1, cp // 2)
            p = np.concatenate([[N], (rd + i) % N])
            q = np.concatenate([[rd], (rd - i + N) % N])
            ap, aq = a[:, p], a[:, q]
            alpha, beta, gam = (ap * ap).sum(0), (aq * aq).sum(0), (ap * aq).sum(0)
            ab = alpha * beta
            rot = (ab > 0) & (np.abs(gam) > 2.0 ** -50 * np.sqrt(ab))
            if not rot.any():
                continue
            zeta = (beta - alpha) / (2.0 * np.where(rot, gam, 1.0))
            t = np.where(zeta == 0, 1.0, np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta)))
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sn = cs * t
            cs, sn = np.where(rot, cs, 1.0), np.where(rot, sn, 0.0)
            a[:, p], a[:, q] = cs * ap - sn * aq, sn * ap + cs * aq
            rotations += int(rot.sum())
        if rotations == 0:
            return np.sqrt((a[:, :c] ** 2).sum(0)), sweep
    raise RuntimeError(f"no convergence in {max_sweeps} sweeps")
