"""Witness of the lockstep BFGS: the vector form of one window's minimisation as the product held it before the scalar-driven
machine carried both forms (batch_solver._WindowBFGS at that commit, text unchanged but for the two module globals it read, which are
arguments here), and a plain loop equal to LockstepBFGS._run.  Frozen and simple: the package never imports it, and it changes only with
SciPy's own algorithm.  The helper-thread plumbing and the line-search constants come from the product; the algorithm does not.

``exact_max_n``: up to this many unknowns the inverse-Hessian update is SciPy's own expression, above it the rank-two form;
``triangle``: above it the inverse Hessian lives in one triangle (dsymv / dsyr2) - the product does that when it has threadpoolctl,
and ``run`` follows the product's ``threadpool_limits`` at the moment of the call, BLAS on one thread as the product's drivers run it."""
import importlib

import numpy as np
import scipy.optimize as spo
from scipy.optimize._dcsrch import DCSRCH
from scipy.optimize._linesearch import line_search_wolfe2
from scipy.linalg.blas import dsymv, dsyr2

bs = importlib.import_module('edge-informed-contrast-maximization_amd.batch_solver')
_CoroutineCall = bs._CoroutineCall
_BFGS_C1, _BFGS_C2, _BFGS_XTOL, _BFGS_AMIN, _BFGS_AMAX, _LS_MAXITER = (bs._BFGS_C1, bs._BFGS_C2, bs._BFGS_XTOL, bs._BFGS_AMIN,
                                                                        bs._BFGS_AMAX, bs._LS_MAXITER)


class _WindowBFGS:
    """One window's BFGS, one function evaluation at a time (scipy.optimize._optimize._minimize_bfgs with jac=True)."""

    def __init__(self, x0, maxiter, gtol, callback=None, wolfe2_fallback=True, exact_max_n=64, triangle=False):
        self.exact_max_n, self.triangle = int(exact_max_n), bool(triangle)
        self.wolfe2_fallback = bool(wolfe2_fallback)
        self.x0 = np.array(x0, dtype=np.float64).reshape(-1)
        self.n = self.x0.size
        self.maxiter = int(maxiter) if maxiter is not None else self.n * 200
        self.gtol = float(gtol)
        self.callback = callback
        self.phase = 'init'
        self.request = self.x0                  # the point whose (value, grad) this window wants next; None = finished
        self.k = 0
        self.nfev = 0
        self.warnflag = 0
        self.result = None

    # -- what the driver calls ----------------------------------------------------------------------------------
    def feed(self, f, g, single_eval):
        """(value, grad) at ``self.request``.  single_eval(x) -> (f, g) evaluates this window alone (the rare wolfe2 fallback)."""
        self.nfev += 1
        f = float(f)
        g = np.array(g, dtype=np.float64).reshape(-1)
        if self.phase == 'init':
            self.xk, self.old_fval, self.gfk = self.x0, f, g
            self.sym = self.triangle and self.n > self.exact_max_n
            # sym: the inverse Hessian lives in the UPPER triangle of a Fortran-ordered array (dsymv / dsyr2 touch half the matrix)
            self.Hk = np.asfortranarray(np.eye(self.n)) if self.sym else np.eye(self.n)
            self.old_old_fval = self.old_fval + np.linalg.norm(self.gfk) / 2          # initial step guess dx ~ 1
            self.gnorm = np.abs(self.gfk).max() if self.n else 0.0
            self._begin_iteration(single_eval)
        elif self.phase == 'ls':
            self.phi1, self.gval = f, g
            self.derphi1 = float(np.dot(g, self.pk))
            self._ls_step(single_eval)
        elif self.phase == 'ls2':
            self.ls2.answer(f, g)
            self._ls2_advance(single_eval)
        else:
            raise RuntimeError('feed() on a finished window')

    # -- BFGS iteration -------------------------------------------------------------------------------------------
    def _begin_iteration(self, single_eval):
        if not (self.gnorm > self.gtol and self.k < self.maxiter):
            return self._finish()
        self.pk = -dsymv(1.0, self.Hk, self.gfk, lower=0) if self.sym else -np.dot(self.Hk, self.gfk)
        derphi0 = float(np.dot(self.gfk, self.pk))
        # scalar_search_wolfe1: the first trial step
        if self.old_old_fval is not None and derphi0 != 0:
            alpha1 = min(1.0, 1.01 * 2 * (self.old_fval - self.old_old_fval) / derphi0)
            if alpha1 < 0:
                alpha1 = 1.0
        else:
            alpha1 = 1.0
        self.dcsrch = DCSRCH(None, None, _BFGS_C1, _BFGS_C2, _BFGS_XTOL, _BFGS_AMIN, _BFGS_AMAX)
        self.task, self.alpha1, self.phi1, self.derphi1, self.derphi0 = b'START', alpha1, self.old_fval, derphi0, derphi0
        self.gval = self.gfk
        self.ls_iter = 0
        self._ls_step(single_eval)

    def _ls_step(self, single_eval):
        """One pass of the loop of DCSRCH.__call__; leaves a request behind, or ends the line search."""
        if self.ls_iter >= _LS_MAXITER:
            return self._ls_done(None, single_eval)
        self.ls_iter += 1
        stp, self.phi1, self.derphi1, self.task = self.dcsrch._iterate(self.alpha1, self.phi1, self.derphi1, self.task)
        if not np.isfinite(stp):
            return self._ls_done(None, single_eval)
        if self.task[:2] == b'FG':
            self.alpha1 = stp
            self.phase, self.request = 'ls', self.xk + stp * self.pk
            return
        if self.task[:5] == b'ERROR' or self.task[:4] == b'WARN':
            stp = None
        self._ls_done(stp, single_eval)

    def _ls_done(self, stp, single_eval):
        if stp is not None:
            return self._step_taken(stp, self.phi1, self.gval, single_eval)
        if not self.wolfe2_fallback:                               # opt-out of SciPy's second line search: precision loss here and now
            self.warnflag = 2
            return self._finish()
        # _line_search_wolfe12: DCSRCH found no step, SciPy tries its other line search.  That one is not written for reverse
        # communication, so it runs in a helper thread whose f / fprime calls become this window's requests: the evaluations
        # stay in lockstep with the other windows (with the engine's fp32-level noise this fallback is the common end of a level)
        self.ls2 = _CoroutineCall(lambda fv, fg: line_search_wolfe2(fv, fg, self.xk, self.pk, self.gfk, self.old_fval, self.old_old_fval,
                                                                     c1=_BFGS_C1, c2=_BFGS_C2, amax=_BFGS_AMAX))
        self._ls2_advance(single_eval)

    def _ls2_advance(self, single_eval):
        kind, payload = self.ls2.next()
        if kind == 'request':
            self.phase, self.request = 'ls2', payload
            return
        ret = payload
        if ret[0] is None:
            self.warnflag = 2                                      # precision loss: no step satisfies the Wolfe conditions
            return self._finish()
        alpha_k, new_fval, gfkp1 = ret[0], ret[3], ret[5]
        if gfkp1 is None:                                          # (line_search_wolfe2 returns the gradient of its last evaluation)
            gfkp1 = np.asarray(single_eval(self.xk + alpha_k * self.pk)[1], dtype=np.float64).reshape(-1)
        self._step_taken(alpha_k, new_fval, gfkp1, single_eval)

    def _step_taken(self, alpha_k, new_fval, gfkp1, single_eval):
        self.old_fval, self.old_old_fval = new_fval, self.old_fval
        sk = alpha_k * self.pk
        self.xk = self.xk + sk
        yk = gfkp1 - self.gfk
        self.gfk = gfkp1
        self.k += 1
        if self.callback is not None:
            self.callback(spo.OptimizeResult(x=self.xk, fun=self.old_fval))
        self.gnorm = np.abs(self.gfk).max()
        if self.gnorm <= self.gtol:
            return self._finish()
        if alpha_k * np.linalg.norm(self.pk) <= 0.0:              # xrtol = 0
            return self._finish()
        if not np.isfinite(self.old_fval):
            self.warnflag = 2
            return self._finish()
        rhok_inv = float(np.dot(yk, sk))
        rhok = 1000.0 if rhok_inv == 0.0 else 1.0 / rhok_inv
        if self.n <= self.exact_max_n:                          # SciPy's own expression (bit for bit the same inverse Hessian)
            I = np.eye(self.n, dtype=int)
            A1 = I - sk[:, np.newaxis] * yk[np.newaxis, :] * rhok
            A2 = I - yk[:, np.newaxis] * sk[np.newaxis, :] * rhok
            self.Hk = np.dot(A1, np.dot(self.Hk, A2)) + (rhok * sk[:, np.newaxis] * sk[np.newaxis, :])
        else:
            # the same update as ONE symmetric rank-two correction, O(n^2) instead of the two n x n products (n = 512 at a 16x16
            # theta: 10 ms per iteration in SciPy's form, the evaluation itself takes 0.1 ms):
            #   (I - r s y^T) H (I - r y s^T) + r s s^T = H - r (s (Hy)^T + (Hy) s^T) + r (1 + r y^T H y) s s^T     (H symmetric)
            #                                         = H + s w^T + w s^T,   w = (c / 2) s - r Hy,  c = r (1 + r y^T H y)
            Hy = dsymv(1.0, self.Hk, yk, lower=0) if self.sym else np.dot(self.Hk, yk)
            w = (0.5 * rhok * (1.0 + rhok * float(np.dot(yk, Hy)))) * sk - rhok * Hy
            if self.sym:
                self.Hk = dsyr2(1.0, sk, w, a=self.Hk, overwrite_a=1, lower=0)     # in place, upper triangle
            else:
                sw = np.outer(sk, w)
                self.Hk = self.Hk + sw + sw.T
        self._begin_iteration(single_eval)

    def _finish(self):
        fval = self.old_fval
        if self.warnflag == 2:
            pass
        elif self.k >= self.maxiter:
            self.warnflag = 1
        elif np.isnan(self.gnorm) or np.isnan(fval) or np.isnan(self.xk).any():
            self.warnflag = 3
        self.phase, self.request = 'done', None
        if getattr(self, 'sym', False):                             # hand out the full matrix
            d = self.Hk.diagonal().copy()                          # (the strictly lower triangle is still the identity's: zero)
            self.Hk = self.Hk + self.Hk.T
            self.Hk[np.diag_indices(self.n)] = d
            self.sym = False
        self.result = spo.OptimizeResult(fun=fval, jac=self.gfk, hess_inv=self.Hk, nfev=self.nfev, njev=self.nfev,
                                         status=self.warnflag, success=(self.warnflag == 0), x=self.xk, nit=self.k)


class Counts:
    n_batch_evals = n_window_evals = 0


def run(fun_batch, x0, maxiter, gtol, exact_max_n, callbacks=None, active=None, wolfe2_fallback=True, counts=None):
    """B minimisations in lockstep: list of scipy OptimizeResult (None for inactive windows).  ``counts``: a Counts to fill."""
    x0 = np.asarray(x0, dtype=np.float64)
    B = x0.shape[0]
    act = np.ones(B, bool) if active is None else np.asarray(active, bool)
    cbs = callbacks if callbacks is not None else [None] * B
    limits = bs.threadpool_limits
    windows = [(_WindowBFGS(x0[b], maxiter, gtol, cbs[b], wolfe2_fallback, exact_max_n, limits is not None) if act[b] else None)
               for b in range(B)]
    last = x0.copy()
    counts = counts if counts is not None else Counts()

    def single(b):
        def ev(x):
            X = last.copy()
            X[b] = np.asarray(x, dtype=np.float64).reshape(-1)
            m = np.zeros(B, bool); m[b] = True
            counts.n_batch_evals += 1; counts.n_window_evals += 1
            v, g = fun_batch(X, m)
            return float(v[b]), np.array(g[b], dtype=np.float64)
        return ev

    def loop():
        while True:
            req = [(b, w) for b, w in enumerate(windows) if w is not None and w.request is not None]
            if not req:
                break
            m = np.zeros(B, bool)
            for b, w in req:
                last[b] = w.request
                m[b] = True
            counts.n_batch_evals += 1; counts.n_window_evals += len(req)
            v, g = fun_batch(last, m)
            for b, w in req:
                w.feed(v[b], g[b], single(b))
        return [w.result if w is not None else None for w in windows]
    try:
        if limits is not None:
            with limits(limits=1, user_api='blas'):
                return loop()
        return loop()
    finally:
        for w in windows:
            ls2 = getattr(w, 'ls2', None) if w is not None else None
            if ls2 is not None:
                ls2.abandon()
