"""NumPy restatement of the reference's lanczos_periodic and lanczos_selective
(lanczos.m:136-311), the two modes the oracle's ``lanczos`` leaves out.  Built
on the oracle's projectAndNormalize, normest and matlab_eig; the recurrence
lines are the oracle's lanczos_basic, so a run in which no event fires gives
its 'local' T and Q bit for bit.

One deliberate difference, shared with the library: for j <= 6 the reference's
window Q(:,j-5:j+1) indexes out of range; here it is clamped to start at
column 1 and the earlier block is then empty.
"""
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import ca_lanczos_ref as ref

EPS = np.finfo(float).eps


def update_omega(omega_in, n, alpha, beta, anorm):
    """lanczos.m:267-300; n, alpha(i), beta(i) are MATLAB's (1-based)."""
    T = EPS * anorm
    al = lambda i: alpha[i - 1]      # noqa: E731
    be = lambda i: beta[i - 1]       # noqa: E731
    binv = 1.0 / be(n)
    om = np.zeros((n + 1, n + 1))
    if omega_in is None or omega_in.size == 0:
        om[0, 0] = 1.0
        om[0, 1] = 0.0
        om[1, 0] = binv * T
        om[1, 1] = 1.0
        return om
    om[:n, :n] = omega_in
    O = lambda i, k: om[i - 1, k - 1]    # noqa: E731
    v = be(2) * O(n, 2) + (al(1) - al(n)) * O(n, 1) - be(n) * O(n - 1, 1)
    om[n, 0] = binv * (v + T) if v > 0 else binv * (v - T)
    for k in range(2, n):
        v = be(k + 1) * O(n, k + 1) + (al(k) - al(n)) * O(n, k) + be(k) * O(n, k - 1) - be(n) * O(n - 1, k)
        om[n, k - 1] = binv * (v + T) if v > 0 else binv * (v - T)
    om[n, n - 1] = binv * T
    om[n, n] = 1.0
    return om


def reset_omega(omega_in, n, anorm):
    """lanczos.m:302-311: rows n and n+1."""
    om = omega_in.copy()
    T = EPS * anorm
    om[n - 1, :n] = T
    om[n, :n] = T
    om[n - 1, n - 1] = 1.0
    om[n - 1, n] = 0.0
    om[n, n] = 1.0
    return om


@dataclass
class StdLanczosRef:
    T: np.ndarray
    Q: np.ndarray
    alpha: np.ndarray
    beta: np.ndarray
    events: list = field(default_factory=list)   # periodic: steps; selective: (step, locked)
    margins: list = field(default_factory=list)  # per step: the decision's value / its threshold
    norm_A: float = 0.0


def _recurrence(A, Q, alpha, beta, j):
    r = A @ Q[:, j]                                             # :155 / :226
    if j > 0:
        r = r - beta[j - 1] * Q[:, j - 1]
    alpha[j] = r @ Q[:, j]
    r = r - alpha[j] * Q[:, j]
    beta[j] = math.sqrt(r @ r)
    Q[:, j + 1] = r / beta[j]


def lanczos_periodic(A, r, maxiter):
    q = r / np.linalg.norm(r)                                   # :47
    n = len(q)
    Q = np.zeros((n, maxiter + 1))
    Q[:, 0] = q
    alpha, beta = np.zeros(maxiter), np.zeros(maxiter)
    norm_A = ref.normest(A)                                     # :219
    omega = None
    out = StdLanczosRef(None, None, alpha, beta, norm_A=norm_A)
    for j in range(maxiter):
        _recurrence(A, Q, alpha, beta, j)
        j1 = j + 1
        omega = update_omega(omega, j1, alpha, beta, norm_A)    # :248
        err = float(np.max(np.abs(omega[j1, :j1])))             # :250
        out.margins.append(err / math.sqrt(EPS))
        if err >= math.sqrt(EPS):                               # :251
            out.events.append(j1)
            first = max(j1 - 6, 0)                              # 0-based first column of the window
            prev = [Q[:, :first]] if first > 0 else []
            QZ, _ = ref.projectAndNormalize(prev, Q[:, first : j1 + 1].copy(), True)   # :253
            Q[:, first : j1 + 1] = QZ
            omega = reset_omega(omega, j1, norm_A)              # :254
    out.T = np.diag(alpha) + np.diag(beta[:-1], 1) + np.diag(beta[:-1], -1)   # :260
    out.Q = Q[:, :maxiter]
    return out


def lanczos_selective(A, r, maxiter):
    q = r / np.linalg.norm(r)
    n = len(q)
    Q = np.zeros((n, maxiter + 1))
    QR = np.zeros((n, maxiter))
    Q[:, 0] = q
    alpha, beta = np.zeros(maxiter), np.zeros(maxiter)
    norm_A = ref.normest(A)                                     # :146
    thr = norm_A * math.sqrt(EPS)
    nritz = 0
    out = StdLanczosRef(None, None, alpha, beta, norm_A=norm_A)
    for j in range(maxiter):
        _recurrence(A, Q, alpha, beta, j)
        j1 = j + 1
        Tj = np.diag(alpha[:j1]) + np.diag(beta[:j], 1) + np.diag(beta[:j], -1)   # :164
        _, Vp = ref.matlab_eig(Tj)
        vals = np.array([beta[i] * abs(Vp[j1 - 1, i]) for i in range(j1)])         # :168 (beta(i), literally)
        conv = [i for i in range(j1) if vals[i] < thr]
        # the decision nearest its threshold among those that would change the count
        out.margins.append(float(np.min(np.abs(vals / thr - 1.0))))
        if len(conv) > nritz:                                   # :172
            nritz = len(conv)
            for k, i in enumerate(conv):
                QR[:, k] = Q[:, :j1] @ Vp[:, i]                 # :178-179
            out.events.append((j1, nritz))
        if nritz > 0:                                           # :183-185
            QZ, _ = ref.projectAndNormalize([QR[:, :nritz]], Q[:, j1 : j1 + 1].copy(), False)
            Q[:, j1] = QZ[:, 0]
    out.T = np.diag(alpha) + np.diag(beta[:-1], 1) + np.diag(beta[:-1], -1)
    out.Q = Q[:, :maxiter]
    return out


def lanczos(A, r, maxiter, orth):
    o = orth.lower()
    if o == "periodic":
        return lanczos_periodic(A, r, maxiter)
    if o == "selective":
        return lanczos_selective(A, r, maxiter)
    raise ValueError("lanczos_std_ref restates 'periodic' and 'selective' only: %s" % orth)


def diag_test_matrix():
    """A = diag([linspace(0,1,1190), 2, 2.5, 3, 4]) as CSR (n = 1194), ||A|| = 4."""
    import scipy.sparse as sp

    d = np.concatenate([np.linspace(0.0, 1.0, 1190), [2.0, 2.5, 3.0, 4.0]])
    return sp.diags(d, format="csr")
