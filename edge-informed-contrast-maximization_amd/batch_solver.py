"""Lockstep solver for a BATCH of independent event windows: the caller of the engine's batch path (BASELINE config C4).

The reference solves one window at a time (upstream src/eincm/solver.py:197-267, src/experiments/e00/exp_mgr.py:615-659):
every BFGS function evaluation is one loss+grad of one window.  The HIP engine evaluates B windows in ONE call at 2-3 times the
per-window rate of B single calls (bench.py: 8 x 10^6 events in 0.24 ms against 8 x 0.07 ms), but only a caller that has B thetas
ready at the same moment can use that.  This module is that caller:

* ``LockstepBFGS`` runs B independent BFGS minimisations - SciPy's own algorithm (scipy.optimize._optimize._minimize_bfgs: inverse
  Hessian update, initial step guess, strong-Wolfe line search by MINPACK's DCSRCH with the fallback to line_search_wolfe2, the same
  stopping rules and status codes), restated as a state machine that asks for ONE function evaluation at a time - and answers all
  the requests of a tick with one batched evaluation.  Windows that have converged ride along with their last theta.  Given the
  same (value, grad) a window takes exactly the steps SciPy's BFGS would take.
* The algorithm is restated once, in ``_BFGSMachine``, which sees scalars only; the vectors of a window are a ``_HostWindow`` (numpy:
  the three forms of the inverse-Hessian update, each written once) or rows of the GPU's state.  ``LockstepBFGS`` drives the machine
  through ``_WindowBFGS`` (machine + host window, asks for points), ``DeviceLockstepBFGS`` drives it over a state object
  (``NumpyBFGSState``: B host windows, the written contract of ``DeviceBFGSState``).  tests/_bfgs_witness.py holds both to a frozen
  vector form of the algorithm, bit for bit.
* ``BatchedMultipleLevelEINCMSolver`` drives the theta pyramid of B windows (or of the current windows of B independent sequences)
  level by level with it: same constructor keywords, state and per-window result dict as ``solver.MultipleLevelEINCMSolver``
  (reference solver.py:16-126, :254-267), retries included; a solved handover weight (L-BFGS-B on one scalar, :325-335) is found
  window by window with the other windows riding along.
"""
import math

import numpy as np
import scipy.optimize as spo
from scipy.optimize._dcsrch import DCSRCH            # MINPACK-2 dcsrch as SciPy ships it: reverse communication, one step per call
from scipy.optimize._linesearch import line_search_wolfe2, scalar_search_wolfe2
from scipy.linalg.blas import dsymv, dsyr2

if not hasattr(DCSRCH, '_iterate'):                  # private SciPy API (1.12 ... 1.15 have it): fail at import, not mid-solve
    raise ImportError('batch_solver needs scipy.optimize._dcsrch.DCSRCH._iterate (SciPy >= 1.12); found SciPy ' + __import__('scipy').__version__)

try:                                                 # level-2 BLAS on a 512 x 512 matrix must not fan out over the host's cores
    import threadpoolctl                             # (OpenBLAS with 8+ threads: 15 ms per dsyr2 instead of 0.1 ms)
    _TPC = [None]

    def threadpool_limits(limits, user_api):
        """threadpoolctl's limiter on ONE controller per process: building a controller walks every loaded shared library (2 ms
        with torch in the process); limiting through an existing one takes 10 us."""
        if _TPC[0] is None:
            _TPC[0] = threadpoolctl.ThreadpoolController()
        return _TPC[0].limit(limits=limits, user_api=user_api)
except ImportError:                                  # without it the update stays in plain numpy
    threadpool_limits = None

from . import _lib as L
from .engine import Engine, check_history, check_initial_scale, check_precision, check_window_size, make_params
from .solver import ScipyMinimizeInfo, EmptyCallback, rescale_theta, _canon, advect_theta_pyramids, prior_transport_settings

_BFGS_C1, _BFGS_C2, _BFGS_XTOL, _BFGS_AMIN, _BFGS_AMAX, _LS_MAXITER = 1e-4, 0.9, 1e-14, 1e-100, 1e100, 100
_EXACT_UPDATE_MAX_N = 64          # up to this many unknowns the inverse-Hessian update is SciPy's own expression (two n x n products)


class _QuietLineSearch:
    """``warnings.catch_warnings`` is process-wide state: helper threads that enter and leave it independently restore each other's
    filters (the first one out switches the warning back on for the others).  This one counts: the first thread in installs the
    filter for scipy's LineSearchWarning, the last one out restores what was there."""

    def __init__(self):
        import threading
        self._lock, self._n, self._cw = threading.Lock(), 0, None

    def __enter__(self):
        import warnings
        from scipy.optimize._linesearch import LineSearchWarning
        with self._lock:
            if self._n == 0:
                self._cw = warnings.catch_warnings()
                self._cw.__enter__()
                warnings.simplefilter('ignore', LineSearchWarning)
            self._n += 1

    def __exit__(self, *exc):
        with self._lock:
            self._n -= 1
            if self._n == 0:
                self._cw.__exit__(None, None, None)
                self._cw = None
        return False


_quiet_line_search = _QuietLineSearch()


class _Abandoned(BaseException):
    """Raised inside a helper thread whose owner abandoned the minimisation."""


class _CoroutineCall:
    """Runs target(f, fprime) in a helper thread and turns its calls of f(x) / fprime(x) into requests the owner answers:
    next() -> ('request', x) or ('done', result); answer(value, grad) resumes the target.  One of the two threads runs at a time."""

    def __init__(self, target):
        import threading
        self._cv = threading.Condition()
        self._req = self._ans = self._res = None
        self._state = 'running'                  # running | waiting (a request is posted) | done
        self._cache = None

        def f(x):
            x = np.array(x, dtype=np.float64, copy=True)
            with self._cv:
                self._req, self._state = x, 'waiting'
                self._cv.notify_all()
                self._cv.wait_for(lambda: self._state in ('running', 'aborted'))
                if self._state == 'aborted':
                    raise _Abandoned()
                v, g = self._ans
            self._cache = (x, g)
            return v

        def fp(x):
            if self._cache is not None and np.array_equal(self._cache[0], x):
                return self._cache[1]
            f(x)
            return self._cache[1]

        def run():
            try:
                with _quiet_line_search:                        # (SciPy's BFGS silences the fallback's LineSearchWarning too)
                    res = target(f, fp)
            except BaseException as e:          # noqa: BLE001 - handed to the owner
                res = e
            with self._cv:
                self._res, self._state = res, 'done'
                self._cv.notify_all()
        self._thread = threading.Thread(target=run, daemon=True)
        self._thread.start()

    def next(self):
        with self._cv:
            self._cv.wait_for(lambda: self._state in ('waiting', 'done'))
            if self._state == 'waiting':
                return 'request', self._req
        self._thread.join()
        if isinstance(self._res, BaseException):
            raise self._res
        return 'done', self._res

    def answer(self, value, grad):
        with self._cv:
            self._ans = (float(value), np.array(grad, dtype=np.float64).reshape(-1))
            self._state = 'running'
            self._cv.notify_all()

    def abandon(self):
        """The owner gives up (an evaluation raised): wake the helper with an exception so that its thread ends instead of waiting forever."""
        with self._cv:
            if self._state == 'done':
                return
            self._state = 'aborted'
            self._cv.notify_all()
        self._thread.join(timeout=5.0)


class _BFGSMachine:
    """One window's BFGS (scipy.optimize._optimize._minimize_bfgs with jac=True), one function evaluation at a time and with the vectors
    taken out: the phases, the DCSRCH loop, the fallback to SciPy's second line search, the stopping rules and status codes - the only
    restatement of the algorithm; both drivers run it.  x, its gradient g, the direction p and the inverse Hessian live in a state
    (``_HostWindow`` per window, ``NumpyBFGSState``, ``DeviceBFGSState``); the machine is fed (phi, phi' = grad . p, max|grad|) at the step
    it asked for.  ``request`` is that step along p (a float) or None; after a feed ``pending`` may hold (mode, alpha): what the state has
    to do with the window (_lib.BFGS_INIT / UPDATE / MOVE) before ``accepted`` gets the new iterate's scalars.  ``phase``:
    'init' | 'ls' (DCSRCH) | 'ls2' (the fallback, ``ls2`` its helper thread) | 'reeval' | 'done'."""

    def __init__(self, maxiter, gtol, n, wolfe2_fallback=True):
        self.wolfe2_fallback = bool(wolfe2_fallback)
        self.n = int(n)
        self.maxiter = int(maxiter) if maxiter is not None else self.n * 200
        self.gtol = float(gtol)
        self.phase, self.request = 'init', 0.0          # the first evaluation: at x0 (the state's direction is 0)
        self.pending = None
        self.k = self.nfev = self.warnflag = 0
        self.ls2 = None

    def feed(self, f, dphi, gmax):
        f, dphi, gmax = float(f), float(dphi), float(gmax)
        if self.phase == 'init':
            self.nfev += 1
            self.old_fval, self.gnorm = f, gmax
            self._after = 'init'
            self.pending, self.request = (L.BFGS_INIT, 0.0), None
        elif self.phase == 'ls':
            self.nfev += 1
            self.phi1, self.derphi1, self.gmax_t = f, dphi, gmax
            self._ls_step()
        elif self.phase == 'ls2':
            self.nfev += 1
            self.gmax_t = gmax
            self.ls2.answer(f, dphi)
            self._ls2_advance()
        elif self.phase == 'reeval':                    # the accepted step was not the last one evaluated: its gradient, not counted
            self.gmax_t = gmax
            self._step_taken(self.alpha_k, self.new_fval)
        else:
            raise RuntimeError('feed() on a finished window')

    def accepted(self, scal):
        """The scalars of the iterate the state has just moved to (what ``pending`` asked for)."""
        self.pending, self.scal = None, scal
        if self._after == 'init':
            self.old_old_fval = self.old_fval + scal[L.BFGS_S_GNORM] / 2          # initial step guess dx ~ 1
        if self._after == 'finish':
            return self._finish()
        self._begin_iteration()

    def _begin_iteration(self):
        if not (self.gnorm > self.gtol and self.k < self.maxiter):
            return self._finish()
        derphi0 = float(self.scal[L.BFGS_S_DPHI0])
        self.pnorm = self.scal[L.BFGS_S_PNORM]
        if self.old_old_fval is not None and derphi0 != 0:
            alpha1 = min(1.0, 1.01 * 2 * (self.old_fval - self.old_old_fval) / derphi0)
            if alpha1 < 0:
                alpha1 = 1.0
        else:
            alpha1 = 1.0
        self.dcsrch = DCSRCH(None, None, _BFGS_C1, _BFGS_C2, _BFGS_XTOL, _BFGS_AMIN, _BFGS_AMAX)
        self.task, self.alpha1, self.phi1, self.derphi1, self.derphi0 = b'START', alpha1, self.old_fval, derphi0, derphi0
        self.gmax_t = self.gnorm
        self.ls_iter = 0
        self._ls_step()

    def _ls_step(self):
        if self.ls_iter >= _LS_MAXITER:
            return self._ls_done(None)
        self.ls_iter += 1
        stp, self.phi1, self.derphi1, self.task = self.dcsrch._iterate(self.alpha1, self.phi1, self.derphi1, self.task)
        if not math.isfinite(stp):
            return self._ls_done(None)
        if self.task[:2] == b'FG':
            self.alpha1 = stp
            self.phase, self.request = 'ls', float(stp)
            return
        if self.task[:5] == b'ERROR' or self.task[:4] == b'WARN':
            stp = None
        self._ls_done(stp)

    def _ls_done(self, stp):
        if stp is not None:
            return self._step_taken(stp, self.phi1)
        if not self.wolfe2_fallback:                               # opt-out of SciPy's second line search: precision loss here and now
            self.warnflag = 2
            return self._finish()
        # _line_search_wolfe12: DCSRCH found no step, SciPy tries its other line search (with the engine's fp32-level noise this fallback
        # is the common end of a level).  That one, line_search_wolfe2, is scalar_search_wolfe2 on phi(a) = f(xk + a pk) and
        # derphi(a) = grad . pk with the gradient of the last derphi call kept for the caller.  It is not written for reverse
        # communication, so it runs in a helper thread whose f / fprime calls become this window's requests (_CoroutineCall) and stay in
        # lockstep with the other windows: the point is the step a, the "gradient" phi'(a); the cache answers derphi(a) after phi(a)
        # without an evaluation.
        def search(fv, fg):
            return scalar_search_wolfe2(lambda a: fv(a), lambda a: fg(a)[0], self.old_fval, self.old_old_fval, self.derphi0,
                                        _BFGS_C1, _BFGS_C2, _BFGS_AMAX, None, maxiter=10)
        self.ls2 = _CoroutineCall(search)
        self._ls2_advance()

    def _ls2_advance(self):
        kind, payload = self.ls2.next()
        if kind == 'request':
            self.phase, self.request = 'ls2', float(payload)
            return
        alpha_star, phi_star, _, derphi_star = payload
        if alpha_star is None:
            self.warnflag = 2                                      # precision loss: no step satisfies the Wolfe conditions
            return self._finish()
        if derphi_star is None:                                    # (the search ran out of iterations: its last evaluation was elsewhere)
            self.alpha_k, self.new_fval = float(alpha_star), phi_star
            self.phase, self.request = 'reeval', float(alpha_star)
            return
        self._step_taken(float(alpha_star), phi_star)

    def _step_taken(self, alpha_k, new_fval):
        """The state's trial point is x + alpha_k p and its trial gradient the gradient there."""
        self.old_fval, self.old_old_fval = new_fval, self.old_fval
        self.k += 1
        self.gnorm = self.gmax_t
        self.request = None
        if self.gnorm <= self.gtol or alpha_k * self.pnorm <= 0.0:      # converged / xrtol = 0: SciPy stops before it updates H
            self._after, self.pending = 'finish', (L.BFGS_MOVE, alpha_k)
        elif not math.isfinite(self.old_fval):
            self.warnflag = 2
            self._after, self.pending = 'finish', (L.BFGS_MOVE, alpha_k)
        else:
            self._after, self.pending = 'iterate', (L.BFGS_UPDATE, alpha_k)
        self.stepped = True

    def _finish(self):
        if self.warnflag == 2:
            pass
        elif self.k >= self.maxiter:
            self.warnflag = 1
        elif math.isnan(self.gnorm) or math.isnan(self.old_fval) or math.isnan(self.scal[L.BFGS_S_XMAX]):
            self.warnflag = 3
        self.phase, self.request = 'done', None


def _max_abs(v):
    return np.abs(v).max() if v.size else 0.0


class _HostWindow:
    """One window's vectors on the host: the point x, its gradient g, the direction p, the inverse Hessian H, the trial point
    xt = x + a p of the last evaluation and its gradient gt.  ``form`` is how H is kept and updated:

    * 'exact'  dense, SciPy's own expression (two n x n products): bit for bit SciPy's inverse Hessian
    * 'rank2'  dense, the same update as ONE symmetric rank-two correction, O(n^2) (n = 512 at a 16x16 theta: 10 ms per iteration in
               SciPy's form, the evaluation itself takes 0.1 ms):
                 (I - r s y^T) H (I - r y s^T) + r s s^T = H - r (s (Hy)^T + (Hy) s^T) + r (1 + r y^T H y) s s^T     (H symmetric)
                                                         = H + s w^T + w s^T,   w = (c / 2) s - r Hy,  c = r (1 + r y^T H y)
    * 'tri'    that correction on the UPPER triangle of a Fortran-ordered array (dsymv / dsyr2 touch half the matrix)
    * None     a rider: a point and no H"""

    def __init__(self, x0, form):
        self.form = form
        self.x = self.xt = np.array(x0, dtype=np.float64).reshape(-1)      # (every vector is replaced, never written into)
        self.n = self.x.size
        self.g = self.gt = self.p = np.zeros(self.n)
        self.H = None if form is None else np.asfortranarray(np.eye(self.n)) if form == 'tri' else np.eye(self.n)
        self.I = np.eye(self.n, dtype=int) if form == 'exact' else None      # (SciPy builds it anew in every iteration)

    def trial(self, a):
        self.xt = self.x + a * self.p
        return self.xt

    def take(self, g):
        """The gradient at the trial point -> (gt . p, max|gt|)."""
        self.gt = np.array(g, dtype=np.float64).reshape(-1)
        return float(np.dot(self.gt, self.p)), _max_abs(self.gt)

    def _H_times(self, v):
        return dsymv(1.0, self.H, v, lower=0) if self.form == 'tri' else np.dot(self.H, v)

    def accept(self, alpha, mode, every_scalar=True):
        """_lib.BFGS_UPDATE (the update with s = alpha p, y = gt - g, then x <- xt, g <- gt, p = -H g) / MOVE (x <- xt, g <- gt) / INIT
        (MOVE and p = -H g) -> the _lib.BFGS_NS scalars of the new iterate (y . Hy is 0 in SciPy's form, which never has H y).
        ``every_scalar=False``: only what ``_BFGSMachine.accepted`` reads (g . p, |p|, max|x|, and |g| at INIT), the others 0."""
        ys = yhy = 0.0
        if mode == L.BFGS_UPDATE:
            sk, yk = alpha * self.p, self.gt - self.g
            ys = float(np.dot(yk, sk))
            rhok = 1000.0 if ys == 0.0 else 1.0 / ys
            if self.form == 'exact':
                I = self.I
                A1 = I - sk[:, np.newaxis] * yk[np.newaxis, :] * rhok
                A2 = I - yk[:, np.newaxis] * sk[np.newaxis, :] * rhok
                self.H = np.dot(A1, np.dot(self.H, A2)) + (rhok * sk[:, np.newaxis] * sk[np.newaxis, :])
            else:
                Hy = self._H_times(yk)
                yhy = float(np.dot(yk, Hy))
                w = (0.5 * rhok * (1.0 + rhok * yhy)) * sk - rhok * Hy
                if self.form == 'tri':
                    self.H = dsyr2(1.0, sk, w, a=self.H, overwrite_a=1, lower=0)     # in place, upper triangle
                else:
                    sw = np.outer(sk, w)
                    self.H = self.H + sw + sw.T
        self.x, self.g = self.xt, self.gt
        if mode != L.BFGS_MOVE:
            self.p = -self._H_times(self.g)
        g, p, x = self.g, self.p, self.x
        if every_scalar:
            return (float(np.dot(g, p)), _max_abs(g), np.linalg.norm(p), _max_abs(x), _max_abs(p), np.linalg.norm(g), ys, yhy)
        return (float(np.dot(g, p)), 0.0, np.linalg.norm(p), _max_abs(x), 0.0, np.linalg.norm(g) if mode == L.BFGS_INIT else 0.0, ys, yhy)

    def full_hess_inv(self):
        """The full symmetric matrix, the caller's own."""
        if self.form is None:
            return np.zeros((self.n, self.n))
        if self.form != 'tri':
            return self.H.copy()
        d = self.H.diagonal().copy()                               # (the strictly lower triangle is still the identity's: zero)
        H = self.H + self.H.T
        H[np.diag_indices(self.n)] = d
        return H


class _WindowBFGS:
    """The machine and one host state behind what ``LockstepBFGS`` drives: ``request`` is the POINT whose (value, grad) the window wants
    next (None = finished, ``result`` is there), ``feed`` takes them.  Up to _EXACT_UPDATE_MAX_N unknowns H is updated by SciPy's own
    expression, above that in the rank-two form - in one triangle where BLAS can be kept on one thread (both read at the first feed)."""

    def __init__(self, x0, maxiter, gtol, callback=None, wolfe2_fallback=True):
        self.request = np.array(x0, dtype=np.float64).reshape(-1)
        self.machine = _BFGSMachine(maxiter, gtol, self.request.size, wolfe2_fallback)
        self.callback = callback
        self.state = self.result = None

    phase = property(lambda self: self.machine.phase)
    ls2 = property(lambda self: self.machine.ls2)

    def feed(self, f, g, single_eval):
        """(value, grad) at ``self.request``.  single_eval(x) -> (f, g) evaluates this window alone (the rare wolfe2 fallback)."""
        m = self.machine
        if self.request is None:
            raise RuntimeError('feed() on a finished window')
        if self.state is None:
            n = self.request.size
            self.state = _HostWindow(self.request, 'exact' if n <= _EXACT_UPDATE_MAX_N else 'tri' if threadpool_limits is not None else 'rank2')
        st = self.state
        m.feed(f, *st.take(g))
        if m.phase == 'reeval':                  # the accepted step's gradient, here and now (its value is known; not counted in nfev)
            m.feed(np.nan, *st.take(single_eval(st.trial(m.request))[1]))
        if m.pending is not None:
            mode, alpha = m.pending
            scal = st.accept(alpha, mode, every_scalar=False)
            if mode != L.BFGS_INIT and self.callback is not None:
                self.callback(spo.OptimizeResult(x=st.x, fun=m.old_fval))
            m.accepted(scal)
        if m.request is not None:
            self.request = st.trial(m.request)
            return
        self.request = None
        self.result = spo.OptimizeResult(fun=m.old_fval, jac=st.g, hess_inv=st.full_hess_inv(), nfev=m.nfev, njev=m.nfev,
                                         status=m.warnflag, success=(m.warnflag == 0), x=st.x, nit=m.k)
        self.state = None                                          # (its H is handed out: no second n x n array per finished window)


class LockstepBFGS:
    """B independent BFGS minimisations that evaluate in lockstep.

    fun_batch(X, mask) with X of shape (B, n) returns (values (B,), grads (B, n)); it is called once per tick with every window's
    current request (finished or inactive windows: their last point) and the mask of the windows that asked - the engine evaluates
    only those (Engine.loss_grad(active=...)), so a tick costs what its requesting windows cost.  ``active``: which windows are
    minimised at all.  ``wolfe2_fallback=False`` ends a minimisation with status 2 where DCSRCH finds no step, instead of trying SciPy's
    second line search first (line_search_wolfe2: some 40 evaluations that rarely find a step once the first search has failed on the
    objective's own roughness; profiles/r03/linesearch_fp64_vs_fp32.txt) - a deviation from SciPy, off by default.
    """

    def __init__(self, fun_batch, x0, maxiter, gtol, callbacks=None, active=None, wolfe2_fallback=True, groups=None, launch=None,
                 collect=None):
        """Pipelined form: ``groups`` (index arrays that partition the windows), ``launch(gi, X, mask)`` (enqueue the evaluation of group
        gi's masked windows at X[groups[gi]] and return at once) and ``collect(gi)`` -> (values, grads) of that group.  While the host
        advances the line searches of one group, the other groups' evaluations run on the GPU; ``fun_batch`` is not used then."""
        x0 = np.asarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self.fun_batch = fun_batch
        self.groups = [np.asarray(ix, dtype=int) for ix in groups] if groups is not None else None
        self.launch, self.collect = launch, collect
        if self.groups is not None:
            assert launch is not None and collect is not None
            assert sorted(int(b) for ix in self.groups for b in ix) == list(range(self.B)), 'groups must partition the windows'
            self._group_of = {int(b): gi for gi, ix in enumerate(self.groups) for b in ix}
            self._pos = {int(b): i for ix in self.groups for i, b in enumerate(ix)}
            self._inflight = [None] * len(self.groups)
        act = np.ones(self.B, bool) if active is None else np.asarray(active, bool)
        maxiters = np.broadcast_to(np.asarray(maxiter), (self.B,))
        cbs = callbacks if callbacks is not None else [None] * self.B
        self.windows = [(_WindowBFGS(x0[b], maxiters[b], gtol, cbs[b], wolfe2_fallback) if act[b] else None) for b in range(self.B)]
        self.last = x0.copy()
        self.n_batch_evals = 0                  # engine calls
        self.n_window_evals = 0                 # windows evaluated over all calls

    def _single(self, b):
        def ev(x):
            X = self.last.copy()
            X[b] = np.asarray(x, dtype=np.float64).reshape(-1)
            m = np.zeros(self.B, bool); m[b] = True
            self.n_batch_evals += 1; self.n_window_evals += 1
            if self.groups is not None:                 # (called while group gi is being fed: its context is idle)
                gi = self._group_of[b]
                self.launch(gi, X, m)
                v, g = self.collect(gi)
                return float(v[self._pos[b]]), np.array(g[self._pos[b]], dtype=np.float64)
            v, g = self.fun_batch(X, m)
            return float(v[b]), np.array(g[b], dtype=np.float64)
        return ev

    def run(self):
        """List of scipy OptimizeResult (None for inactive windows)."""
        run = self._run if self.groups is None else self._run_pipelined
        try:
            if threadpool_limits is not None:
                with threadpool_limits(limits=1, user_api='blas'):
                    return run()
            return run()
        finally:                                   # an evaluation raised mid-solve: no helper thread of a line-search fallback stays behind
            if self.groups is not None:            # ... and no evaluation in flight
                for gi, req in enumerate(self._inflight):
                    if req is not None:
                        self._inflight[gi] = None
                        try:
                            self.collect(gi)
                        except Exception:          # noqa: BLE001 - the first error is the one that propagates
                            pass
            for w in self.windows:
                ls2 = getattr(w, 'ls2', None) if w is not None else None
                if ls2 is not None:
                    ls2.abandon()

    def _run(self):
        while True:
            req = [(b, w) for b, w in enumerate(self.windows) if w is not None and w.request is not None]
            if not req:
                break
            m = np.zeros(self.B, bool)
            for b, w in req:
                self.last[b] = w.request
                m[b] = True
            self.n_batch_evals += 1; self.n_window_evals += len(req)
            v, g = self.fun_batch(self.last, m)
            for b, w in req:
                w.feed(v[b], g[b], self._single(b))
        return self._results()

    def _results(self):
        for b, w in enumerate(self.windows):          # riders keep their final point in `last`
            if w is not None:
                self.last[b] = w.result.x
        return [w.result if w is not None else None for w in self.windows]

    def _start_group(self, gi):
        req = [(int(b), self.windows[b]) for b in self.groups[gi] if self.windows[b] is not None and self.windows[b].request is not None]
        if not req:
            self._inflight[gi] = None
            return
        m = np.zeros(self.B, bool)
        for b, w in req:
            self.last[b] = w.request
            m[b] = True
        self.n_batch_evals += 1; self.n_window_evals += len(req)
        self.launch(gi, self.last, m)
        self._inflight[gi] = req

    def _run_pipelined(self):
        for gi in range(len(self.groups)):
            self._start_group(gi)
        while any(r is not None for r in self._inflight):
            for gi in range(len(self.groups)):
                req = self._inflight[gi]
                if req is None:
                    continue
                v, g = self.collect(gi)                # waits for group gi; the other groups' evaluations keep running
                self._inflight[gi] = None
                for b, w in req:
                    w.feed(v[self._pos[b]], g[self._pos[b]], self._single(b))
                self._start_group(gi)                  # back on the GPU before the next group is collected and fed
        return self._results()

# ---- the machine driven over a state object: x, its gradient, the direction and the inverse Hessian of all windows live there --------------
BFGS_STATES = ('host', 'device')


def check_bfgs_state(bfgs_state):
    """'host' or 'device'; anything else is a ValueError."""
    if bfgs_state not in BFGS_STATES:
        raise ValueError(f"bfgs_state {bfgs_state!r}: 'host' or 'device'")
    return bfgs_state


class NumpyBFGSState:
    """The state interface on the CPU: B ``_HostWindow`` in the rank-two form (in the triangle wherever BLAS can be kept on one thread) -
    the written-down contract of ``DeviceBFGSState``, op for op what the GPU does.  A state holds, per window, the point x, its gradient
    g, the direction p, the inverse Hessian H, the trial point xt = x + a p of the last evaluation and its gradient gt:

    * ``begin(x0, active)``          x = x0, H = I
    * ``eval(alpha, mask)``          one evaluation at x + alpha[b] p per window of the mask -> (f, phi' = gt . p, max|gt|), each (B,)
    * ``accept(alpha, modes)``       per window _lib.BFGS_SKIP / UPDATE (the rank-two update with s = alpha p, y = gt - g, then x <- xt,
                                     g <- gt, p = -H g) / MOVE (x <- xt, g <- gt) / INIT (MOVE and p = -H g) -> scalars (B, _lib.BFGS_NS)
    * ``fetch(want_hess_inv)``       (x, g, H | None) as arrays (B, n), (B, n), (B, n, n)

    fun_batch(X, mask) -> (values (B,), grads (B, n)) as for ``LockstepBFGS``."""

    def __init__(self, fun_batch):
        self.fun_batch = fun_batch
        self.windows = []

    def _new_window(self, x0):
        return _HostWindow(x0, 'tri' if threadpool_limits is not None else 'rank2')

    def begin(self, x0, active=None):
        x0 = np.array(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        act = np.ones(self.B, bool) if active is None else np.asarray(active, bool)
        if not self.windows or (len(self.windows), self.windows[0].n) != x0.shape:
            self.windows = [_HostWindow(x0[b], None) for b in range(self.B)]
            self.xt = x0.copy()                          # the batch's trial points as fun_batch takes them
            self.scal = np.zeros((self.B, L.BFGS_NS))
        for b in np.flatnonzero(act):
            self.windows[b] = self._new_window(x0[b])

    def _rows(self, name):
        return np.stack([getattr(w, name) for w in self.windows])

    # (B, n) copies of the windows' vectors, for reading: ``set_state`` is the way to write
    x = property(lambda self: self._rows('x'))
    g = property(lambda self: self._rows('g'))
    p = property(lambda self: self._rows('p'))

    def set_state(self, b, x=None, g=None, p=None, H=None):
        """Overwrite parts of window b's state (H: a full symmetric matrix)."""
        w = self.windows[b]
        for name, src in (('x', x), ('g', g), ('p', p)):
            if src is not None:
                setattr(w, name, np.array(src, dtype=np.float64))
        if H is not None:
            H = np.array(H, dtype=np.float64)
            w.H = np.asfortranarray(np.triu(H)) if w.form == 'tri' else H

    def eval(self, alpha, mask):
        for b in np.flatnonzero(mask):
            self.xt[b] = self.windows[b].trial(alpha[b])
        v, g = self.fun_batch(self.xt, mask)
        f, dphi, gmax = np.full(self.B, np.nan), np.zeros(self.B), np.zeros(self.B)
        for b in np.flatnonzero(mask):
            f[b] = float(v[b])
            dphi[b], gmax[b] = self.windows[b].take(g[b])
        return f, dphi, gmax

    def accept(self, alpha, modes):
        for b in range(self.B):
            if int(modes[b]) != L.BFGS_SKIP:
                self.scal[b] = self.windows[b].accept(alpha[b], int(modes[b]))
        return self.scal.copy()

    def full_hess_inv(self, b):
        return self.windows[b].full_hess_inv()

    def fetch(self, want_hess_inv=False):
        return self.x, self.g, (np.stack([w.full_hess_inv() for w in self.windows]) if want_hess_inv else None)


class DeviceBFGSState:
    """The state interface on the GPU: the engine's eincm_bfgs_* entry points (csrc/eincm_bfgs.hip.h).  ``shape``: one window's theta
    (h, w, 2); x0 and the fetched arrays are (B, n) with n = 2 h w.  Nothing but scalars crosses PCIe between begin and fetch."""

    def __init__(self, engine, shape, params):
        self.engine, self.shape, self.params = engine, tuple(shape), params

    def begin(self, x0, active=None):
        x0 = np.asarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self.engine.bfgs_begin(x0.reshape((self.B,) + self.shape), active)

    def eval(self, alpha, mask):
        return self.engine.bfgs_eval(self.params, alpha, mask)

    def accept(self, alpha, modes):
        return self.engine.bfgs_accept(alpha, modes)

    def fetch(self, want_hess_inv=False):
        x, g, H = self.engine.bfgs_fetch(want_hess_inv)
        return x.reshape(self.B, self.n), g.reshape(self.B, self.n), H


# ---- the limited-memory form of the state: a ring of pairs (s, y) per window instead of the matrix ------------------
LBFGS_EPS = 2.220446049250313e-16          # a pair is kept iff y.s > LBFGS_EPS * y.y (the skip rule of SciPy's L-BFGS-B)
HESSIANS = ('dense', 'limited', 'auto')


def check_hessian(hessian):
    """'dense', 'limited' or 'auto'; anything else is a ValueError."""
    if not isinstance(hessian, str) or hessian not in HESSIANS:
        raise ValueError(f"hessian {hessian!r}: 'dense', 'limited' or 'auto'")
    return hessian


def lbfgs_basis(head, count, m):
    """(ring slots of the pairs, oldest first; indices into D and delta of the basis [s_0 .. s_{c-1}, y_0 .. y_{c-1}, g] in its order):
    s of slot k sits at k, y of slot k at m + k, g at 2 m."""
    slots = [(int(head) + i) % m for i in range(int(count))]
    return slots, slots + [m + k for k in slots] + [2 * m]


def lbfgs_delta(D, head, count, m, initial_scale):
    """The two-loop recursion in its dot-matrix form: D (2m+1, 2m+1) with D[u, v] = b_u . b_v -> the coefficients delta (2m+1) of
    p = sum_j delta_j b_j.  Plain float arithmetic, one operation at a time: every sum runs over the basis in its order, one rounded
    product added after the other, exactly what the GPU's coefficient kernel does (its delta equals this bit for bit on the same D)."""
    slots, order = lbfgs_basis(head, count, m)
    c = len(slots)
    Dl = np.asarray(D, dtype=np.float64)[np.ix_(order, order)].tolist()      # the basis' block, in basis order: s at i, y at c + i, g at 2c
    d = [0.0] * (2 * c + 1)
    d[2 * c] = -1.0
    a = [0.0] * c
    for i in reversed(range(c)):
        acc = 0.0
        for u in range(2 * c + 1):
            acc += d[u] * Dl[u][i]
        a[i] = acc / Dl[i][c + i]
        d[c + i] -= a[i]
    if initial_scale == 'last_pair' and c:
        gamma = Dl[c - 1][2 * c - 1] / Dl[2 * c - 1][2 * c - 1]
        for u in range(2 * c + 1):
            d[u] *= gamma
    for i in range(c):
        acc = 0.0
        for u in range(2 * c + 1):
            acc += d[u] * Dl[u][c + i]
        beta = acc / Dl[i][c + i]
        d[i] += a[i] - beta
    delta = np.zeros(2 * m + 1)
    delta[order] = d
    return delta


def lbfgs_combine(delta, S, Y, g, head, count, m):
    """p = sum_j delta_j b_j per element over the basis in its order: the first product as it is, every later one rounded, then added."""
    slots, _ = lbfgs_basis(head, count, m)
    terms = [delta[k] * S[k] for k in slots] + [delta[m + k] * Y[k] for k in slots] + [delta[2 * m] * np.asarray(g)]
    p = terms[0]
    for v in terms[1:]:
        p = p + v
    return p


class _LimitedWindow(_HostWindow):
    """One window's vectors on the host with the inverse Hessian kept as at most m pairs: the rings S, Y (m, n) by ring slot, ``head``
    (the oldest pair's slot), ``count``, the dot matrix D and the coefficients delta (``lbfgs_delta``)."""

    def __init__(self, x0, history, initial_scale):
        super().__init__(x0, None)
        self.form, self.m, self.initial_scale = 'limited', int(history), initial_scale
        m = self.m
        self.S, self.Y = np.zeros((m, self.n)), np.zeros((m, self.n))
        self.D, self.delta = np.zeros((2 * m + 1, 2 * m + 1)), np.zeros(2 * m + 1)
        self.head = self.count = 0

    def _vector(self, u):
        m = self.m
        return self.g if u == 2 * m else self.Y[u - m] if u >= m else self.S[u]

    def _row(self, u):
        """Row (and column) u of D as direct dot products against the whole basis."""
        v = self._vector(u)
        for w in lbfgs_basis(self.head, self.count, self.m)[1]:
            self.D[u, w] = self.D[w, u] = float(np.dot(v, self._vector(w)))

    def accept(self, alpha, mode, every_scalar=True):
        """_lib.BFGS_UPDATE (s = alpha p with the product rounded, y = gt - g; the pair enters the ring iff y.s > LBFGS_EPS y.y, the
        oldest one leaving a full ring; x <- xt, g <- gt; the rows of D of the new s, y and g; delta; p) / MOVE (x <- xt, g <- gt) / INIT
        (MOVE, the ring emptied, p = -g) -> the _lib.BFGS_NS scalars of the new iterate; slot BFGS_S_YHY holds y . y."""
        m = self.m
        ys = yy = 0.0
        kept = None
        if mode == L.BFGS_UPDATE:
            sk, yk = alpha * self.p, self.gt - self.g
            ys, yy = float(np.dot(yk, sk)), float(np.dot(yk, yk))
            if ys > LBFGS_EPS * yy:
                kept = (self.head + self.count) % m
                if self.count == m:
                    self.head = (self.head + 1) % m
                else:
                    self.count += 1
                self.S[kept], self.Y[kept] = sk, yk
        elif mode == L.BFGS_INIT:
            self.head = self.count = 0
            self.D[:] = 0.0
        self.x, self.g = self.xt, self.gt
        if mode != L.BFGS_MOVE:
            if kept is not None:
                self._row(kept)
                self._row(m + kept)
            self._row(2 * m)
            self.delta = lbfgs_delta(self.D, self.head, self.count, m, self.initial_scale)
            self.p = lbfgs_combine(self.delta, self.S, self.Y, self.g, self.head, self.count, m)
        g, p, x = self.g, self.p, self.x
        return (float(np.dot(g, p)), _max_abs(g), np.linalg.norm(p), _max_abs(x), _max_abs(p), np.linalg.norm(g), ys, yy)

    def full_hess_inv(self):
        return None


class NumpyLBFGSState(NumpyBFGSState):
    """``NumpyBFGSState`` with the inverse Hessian of every window kept as a ring of at most ``history`` pairs (s, y): the written-down
    contract of ``DeviceLBFGSState`` (csrc/eincm_lbfgs.hip.h), op for op what the GPU does up to the association of the dot products.
    ``initial_scale``: 'last_pair' starts the recursion from (y.s / y.y) I of the newest pair, 'identity' from I.  There is no inverse
    Hessian to fetch: ``fetch`` returns None for it."""

    def __init__(self, fun_batch, history=10, initial_scale='last_pair'):
        super().__init__(fun_batch)
        self.history, self.initial_scale = check_history(history, None), check_initial_scale(initial_scale)      # (no bound on the host)

    def _new_window(self, x0):
        return _LimitedWindow(x0, self.history, self.initial_scale)

    def full_hess_inv(self, b):
        return None

    def fetch(self, want_hess_inv=False):
        return self.x, self.g, None


class DeviceLBFGSState(DeviceBFGSState):
    """``DeviceBFGSState`` in the limited form (Engine.lbfgs_begin): any theta shape, the dense one included."""

    def __init__(self, engine, shape, params, history=10, initial_scale='last_pair'):
        super().__init__(engine, shape, params)
        self.history, self.initial_scale = check_history(history), check_initial_scale(initial_scale)

    def begin(self, x0, active=None):
        x0 = np.asarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self.engine.lbfgs_begin(x0.reshape((self.B,) + self.shape), active, self.history, self.initial_scale)

    def fetch(self, want_hess_inv=False):
        return super().fetch(False)


class DeviceLockstepBFGS:
    """``LockstepBFGS`` over a state object (``NumpyBFGSState`` / ``DeviceBFGSState``): B scalar-driven minimisations; every tick is one
    ``state.eval`` for all the windows that asked and at most one ``state.accept`` for those whose line search ended.  ``callbacks[b]``
    (or None) gets OptimizeResult(x, fun) per iteration; x crosses to the host before the end only for a callback whose
    ``callback_needs_x[b]`` is true (the default), the others get x=None."""

    def __init__(self, state, x0, maxiter, gtol, callbacks=None, active=None, wolfe2_fallback=True, want_hess_inv=True,
                 callback_needs_x=None):
        x0 = np.asarray(x0, dtype=np.float64)
        self.B, self.n = x0.shape
        self.state, self.x0 = state, x0
        self.active = np.ones(self.B, bool) if active is None else np.asarray(active, bool)
        maxiters = np.broadcast_to(np.asarray(maxiter), (self.B,))
        self.callbacks = callbacks if callbacks is not None else [None] * self.B
        self.needs_x = callback_needs_x if callback_needs_x is not None else [True] * self.B
        self.windows = [(_BFGSMachine(maxiters[b], gtol, self.n, wolfe2_fallback) if self.active[b] else None) for b in range(self.B)]
        self.want_hess_inv = want_hess_inv
        self.n_batch_evals = 0
        self.n_window_evals = 0
        self.n_fetches = 0

    def run(self):
        """List of scipy OptimizeResult (None for inactive windows)."""
        try:
            if threadpool_limits is not None:
                with threadpool_limits(limits=1, user_api='blas'):
                    return self._run()
            return self._run()
        finally:
            for w in self.windows:
                if w is not None and w.ls2 is not None:
                    w.ls2.abandon()

    def _run(self):
        B = self.B
        self.state.begin(self.x0, self.active)
        while True:
            req = [(b, w) for b, w in enumerate(self.windows) if w is not None and w.request is not None]
            if not req:
                break
            alpha, m = np.zeros(B), np.zeros(B, bool)
            for b, w in req:
                alpha[b], m[b] = w.request, True
            self.n_batch_evals += 1; self.n_window_evals += len(req)
            f, dphi, gmax = self.state.eval(alpha, m)
            for b, w in req:
                w.stepped = False
                w.feed(f[b], dphi[b], gmax[b])
            acc = [(b, w) for b, w in req if w.pending is not None]
            if not acc:
                continue
            modes, alpha = np.zeros(B, np.uint8), np.zeros(B)
            for b, w in acc:
                modes[b], alpha[b] = w.pending
            scal = self.state.accept(alpha, modes)
            told = [(b, w) for b, w in acc if w.stepped and self.callbacks[b] is not None]
            if told:
                x = None
                if any(self.needs_x[b] for b, _ in told):
                    self.n_fetches += 1
                    x = self.state.fetch(False)[0]
                for b, w in told:
                    self.callbacks[b](spo.OptimizeResult(x=(x[b].copy() if self.needs_x[b] else None), fun=w.old_fval))
            for b, w in acc:
                w.accepted(scal[b])
        self.n_fetches += 1
        x, g, H = self.state.fetch(self.want_hess_inv)
        out = []
        for b, w in enumerate(self.windows):
            if w is None:
                out.append(None)
                continue
            out.append(spo.OptimizeResult(fun=w.old_fval, jac=g[b].copy(), hess_inv=(H[b].copy() if H is not None else None), nfev=w.nfev,
                                          njev=w.nfev, status=w.warnflag, success=(w.warnflag == 0), x=x[b].copy(), nit=w.k))
        return out


def minimize_thetas(engine, theta0, params, maxiter, gtol, hessian='auto', history=10, bfgs_state='device', callbacks=None, active=None,
                    initial_scale='last_pair', wolfe2_fallback=True, callback_needs_x=None, fun_batch=None, pipeline=None, stats=None):
    """One level of B lockstep BFGS minimisations of the engine's objective over thetas of any shape, the dense one included.

    theta0: (B, h, w, 2).  ``hessian``: 'dense' keeps the n x n inverse Hessian (the device form refuses more than EINCM_BFGS_MAX_N
    unknowns), 'limited' a ring of ``history`` pairs above _EXACT_UPDATE_MAX_N unknowns, 'auto' the matrix up to EINCM_BFGS_MAX_N unknowns
    and the ring above.  ``bfgs_state``: 'device' keeps the vectors in HBM above _EXACT_UPDATE_MAX_N unknowns (DeviceBFGSState /
    DeviceLBFGSState), 'host' in numpy over ``engine.loss_grad`` (LockstepBFGS / NumpyLBFGSState).  ``callbacks[b]`` gets
    OptimizeResult(x (n,), fun) per iteration (x=None where ``callback_needs_x[b]`` is false, device forms only).  ``fun_batch`` /
    ``pipeline`` replace the host forms' evaluation (the multi-context solver's).  ``stats``: a dict whose 'n_batch_evals' and
    'n_window_evals' are advanced.  Returns a list of scipy OptimizeResult (None for inactive windows), x flat."""
    check_hessian(hessian)
    check_bfgs_state(bfgs_state)
    history, initial_scale = check_history(history, L.LBFGS_MAX_HISTORY if bfgs_state == 'device' else None), check_initial_scale(initial_scale)
    theta0 = np.asarray(theta0, dtype=np.float64)
    if theta0.ndim != 4 or theta0.shape[3] != 2:
        raise ValueError(f'theta0 must be (B,h,w,2), got {theta0.shape}')
    B, shape = theta0.shape[0], theta0.shape[1:]
    x = theta0.reshape(B, -1)
    n = x.shape[1]
    limited = n > (_EXACT_UPDATE_MAX_N if hessian == 'limited' else L.BFGS_MAX_N if hessian == 'auto' else n)
    if fun_batch is None:
        def fun_batch(X, mask):
            v, g, _ = engine.loss_grad(X.reshape((B,) + shape), params, active=mask)
            return v, g.reshape(B, -1)
    if bfgs_state == 'device' and n > _EXACT_UPDATE_MAX_N:          # below: the host's bit-exact SciPy update
        state = DeviceLBFGSState(engine, shape, params, history, initial_scale) if limited else DeviceBFGSState(engine, shape, params)
        drv = DeviceLockstepBFGS(state, x, maxiter, gtol, callbacks=callbacks, callback_needs_x=callback_needs_x, active=active,
                                 wolfe2_fallback=wolfe2_fallback, want_hess_inv=False)      # (H stays in HBM: hess_inv is None)
    elif limited:
        drv = DeviceLockstepBFGS(NumpyLBFGSState(fun_batch, history, initial_scale), x, maxiter, gtol, callbacks=callbacks, active=active,
                                 wolfe2_fallback=wolfe2_fallback, want_hess_inv=False)
    else:
        drv = LockstepBFGS(fun_batch, x, maxiter, gtol, callbacks=callbacks, active=active, wolfe2_fallback=wolfe2_fallback, **(pipeline or {}))
    res = drv.run()
    if stats is not None:
        stats['n_batch_evals'] = stats.get('n_batch_evals', 0) + drv.n_batch_evals
        stats['n_window_evals'] = stats.get('n_window_evals', 0) + drv.n_window_evals
    return res


def minimize_motion(engine, model, coeffs0, params, maxiter, gtol, callbacks=None, active=None, wolfe2_fallback=True, stats=None):
    """B lockstep BFGS minimisations of the engine's objective over the coefficients of a parametric motion-field model
    (motion.MotionModel).  coeffs0: (B, K); K <= 12, so every window takes the host's bit-exact SciPy update
    (LockstepBFGS) over ``engine.loss_grad_motion``.  ``callbacks``, ``active``, ``wolfe2_fallback`` and ``stats`` as in minimize_thetas.
    Every step is evaluated by the engine's motion path (Engine.set_motion_path: 'expanded' | 'fused' | 'auto').
    Returns a list of scipy OptimizeResult (None for inactive windows), x the coefficients (K,)."""
    coeffs0 = np.asarray(coeffs0, dtype=np.float64)
    if coeffs0.ndim != 2 or coeffs0.shape[1] != model.n_coeffs:
        raise ValueError(f'coeffs0 must be (B,{model.n_coeffs}), got {coeffs0.shape}')
    if engine.motion_model is not model:
        engine.set_motion_model(model)

    def fun_batch(X, mask):
        v, g, _ = engine.loss_grad_motion(X, params, active=mask)
        return v, g
    drv = LockstepBFGS(fun_batch, coeffs0, maxiter, gtol, callbacks=callbacks, active=active, wolfe2_fallback=wolfe2_fallback)
    res = drv.run()
    if stats is not None:
        stats['n_batch_evals'] = stats.get('n_batch_evals', 0) + drv.n_batch_evals
        stats['n_window_evals'] = stats.get('n_window_evals', 0) + drv.n_window_evals
    return res


def _info(res):
    return ScipyMinimizeInfo(fun_val=float(res.fun), success=bool(res.success), status=int(res.status), iter_num=int(res.nit),
                             hess_inv=getattr(res, 'hess_inv', None), num_fun_eval=int(res.nfev), num_jac_eval=int(res.njev),
                             num_hess_eval=0)


class BatchedMultipleLevelEINCMSolver:
    """The coarse-to-fine theta pyramid of B windows, solved level by level in lockstep on one engine context (or ``n_groups`` of them).

    Constructor keywords follow ``solver.MultipleLevelEINCMSolver`` (reference solver.py:16-126); instead of loss callables it
    takes the loss parameters (``loss_kwargs``: alpha, beta, gamma, delta, scale_to_sensor_size_method[, contrast_kind][, correlation_kind][, tile_size][, window_size][, precision]), because
    the objective is the engine's batched loss+grad.  ``set_datasamples`` stages the B windows (one per sequence, or B independent
    windows); ``solve`` returns one result dict per window with the reference's keys (solver.py:254-267).  Calling set_datasamples /
    solve again continues every sequence with its own prior (handover), exactly as the single-window solver does window after window.
    """

    def __init__(self, n_windows, sensor_size, n_pyr_lvls, theta_opt_maxiters, loss_kwargs, theta_opt_solver_params,
                 handover_opt_maxiters=None, handover_opt_solver_params=None, handover_settings=None,
                 pyramid_downscale_method='bilinear', pyramid_upscale_method='repeat', pyramid_bases=None, device=0,
                 theta_solver_callbacks=None, n_groups=1, bfgs_state='host', hessian='dense', history=10, initial_scale='last_pair'):
        """n_groups > 1: the windows are split over that many engine contexts (HIP streams) and the lockstep is pipelined - while the
        host advances one group's line searches the other groups' evaluations run (LockstepBFGS, pipelined form).
        bfgs_state: 'host' (default) keeps x, the gradient and the inverse Hessian of every window in numpy; 'device' keeps them in HBM
        at the levels with more than 64 unknowns (8x8 and finer: DeviceLockstepBFGS on DeviceBFGSState), where only scalars cross PCIe
        per evaluation; the inverse Hessian of those levels is not downloaded (ScipyMinimizeInfo.hess_inv is None; Engine.bfgs_fetch
        hands it out).  'device' needs one context (n_groups=1) and the fp32 engine.
        hessian: 'dense' (default) keeps the n x n inverse Hessian at every level, so bfgs_state='device' stops at EINCM_BFGS_MAX_N
        unknowns; 'limited' keeps the newest ``history`` pairs (s, y) instead at every level above 64 unknowns (NumpyLBFGSState /
        DeviceLBFGSState; ``initial_scale``: 'last_pair' or 'identity'), which has no bound on the theta shape; 'auto' is dense up to
        EINCM_BFGS_MAX_N unknowns and limited above.  It is the same BFGS machine either way (theta_opt.method stays 'BFGS')."""
        check_bfgs_state(bfgs_state)
        self.hessian, self.initial_scale = check_hessian(hessian), check_initial_scale(initial_scale)
        self.history = check_history(history, L.LBFGS_MAX_HISTORY if bfgs_state == 'device' else None)
        if bfgs_state == 'device' and int(n_groups) > 1:
            raise ValueError("bfgs_state='device' runs on one engine context: n_groups must be 1 (a pipelined device form does not exist)")
        if bfgs_state == 'device' and dict(loss_kwargs).get('precision', 'fp32') == 'fp64':
            raise ValueError("bfgs_state='device' needs precision='fp32': the fp64 engine has no device-resident evaluation")
        self.bfgs_state = bfgs_state
        hs = handover_settings
        if hs is None:
            hs = {'use_handover': False, 'solve_handover_for_levels': [], 'use_downscaled_finest_priors': False,
                  'clip_solved_handover': False, 'alpha_handover': 0.0}
        assert all(k in hs for k in ('use_handover', 'solve_handover_for_levels', 'use_downscaled_finest_priors',
                                     'clip_solved_handover', 'alpha_handover'))
        assert len(theta_opt_maxiters) == n_pyr_lvls, 'theta_opt_maxiters should be provided for each pyramid level'
        assert theta_opt_solver_params['method'] == 'BFGS', 'the lockstep driver restates SciPy BFGS'
        self.B, self.sensor_size, self.n_pyr_lvls = int(n_windows), tuple(sensor_size), int(n_pyr_lvls)
        self.theta_opt_maxiters, self.theta_opt_solver_params = theta_opt_maxiters, theta_opt_solver_params
        self.handover_opt_maxiters = handover_opt_maxiters or {}
        self.handover_opt_solver_params = handover_opt_solver_params
        self.handover_settings = hs
        self.loss_kwargs = dict(loss_kwargs)
        check_precision(self.loss_kwargs.get('precision', 'fp32'))
        if 'window_size' in self.loss_kwargs:
            check_window_size(self.loss_kwargs['window_size'])
        self.pyramid_downscale_method, self.pyramid_upscale_method = pyramid_downscale_method, pyramid_upscale_method
        self.pyramid_bases = pyramid_bases if pyramid_bases is not None else [2] * (n_pyr_lvls - 1)
        self.callbacks = theta_solver_callbacks if theta_solver_callbacks is not None else [EmptyCallback() for _ in range(self.B)]
        self.device = device
        self.n_groups = max(1, min(int(n_groups), self.B))
        self.groups = [np.asarray(ix, dtype=int) for ix in np.array_split(np.arange(self.B), self.n_groups)]
        self.engines = []
        self.engine = None                      # the first group's context (the only one when n_groups == 1)
        self._first = True
        top = np.zeros((1, 1, 2))
        self.prior = [self._pyramid_from_top(top) for _ in range(self.B)]        # prior_theta_pyr per window
        self.n_batch_evals = 0
        self.n_window_evals = 0
        # carrying the priors to the next window: off unless handover_settings asks for it
        self.prior_transport, self._transport_kw = prior_transport_settings(hs)
        self._untransported = None              # the handed-over thetas the held priors were carried from

    def _transported(self, pyrs, **override):
        """The B pyramids carried to the next window, one engine call per level: handover_settings' prior_* values, or
        set_datasamples' (scalars or one per window)."""
        kw = dict(self._transport_kw, **{k: v for k, v in override.items() if v is not None})
        return advect_theta_pyramids(pyrs, self.sensor_size, method=self.loss_kwargs.get('scale_to_sensor_size_method', 'bilinear'),
                                     engine=self.engine, **kw)

    # -- pyramids (solver.py:132-151, :350-377) ---------------------------------------------------------------------
    def _upscale(self, theta, base):
        theta = np.asarray(theta, dtype=np.float64)
        if self.pyramid_upscale_method == 'repeat':
            return np.repeat(np.repeat(theta, base, axis=0), base, axis=1)
        return rescale_theta(theta, (int(theta.shape[0] * base), int(theta.shape[1] * base)), _canon(self.pyramid_upscale_method))

    def _downscale(self, theta, base):
        theta = np.asarray(theta, dtype=np.float64)
        return rescale_theta(theta, (int(theta.shape[0] / base), int(theta.shape[1] / base)), _canon(self.pyramid_downscale_method))

    def _pyramid_from_top(self, top):
        pyr = {f'pyr_lvl_{self.n_pyr_lvls - 1}': np.array(top, copy=True)}
        for k in reversed(range(self.n_pyr_lvls - 1)):
            pyr[f'pyr_lvl_{k}'] = self._upscale(pyr[f'pyr_lvl_{k + 1}'], self.pyramid_bases[-k - 1])
        return pyr

    # -- staging -------------------------------------------------------------------------------------------------------
    def set_datasamples(self, windows, prior_tau=None, prior_gain=None):
        """windows: B tuples (xs, ys, ts, edges, edge_ts), or (xs, ys, ts, edges, edge_ts, weights) with per-event weights or None
        (Engine.set_windows): the tuples go to the engines as they are.  prior_tau / prior_gain
        (prior_transport='advect' only; scalars or one per window): tau and gain of the step that led to THESE windows, for sequences
        with uneven spacing; the priors are carried again from the previous windows' handed-over thetas with them."""
        assert len(windows) == self.B
        if (prior_tau is not None or prior_gain is not None) and self.prior_transport != 'advect':
            raise ValueError("prior_tau / prior_gain need handover_settings['prior_transport'] = 'advect'")
        n_tot = max(sum(len(windows[b][0]) for b in ix) for ix in self.groups)
        R = len(np.atleast_1d(windows[0][4]))
        if not self.engines or n_tot > self._cap or R > self._cap_r:
            self.close()
            self._cap, self._cap_r = max(n_tot, 1), R
            self.engines = [Engine(self.sensor_size, self._cap, max_refs=R, max_windows=len(ix), device=self.device,
                                   precision=self.loss_kwargs.get('precision', 'fp32')) for ix in self.groups]
            self.engine = self.engines[0]
        tiles = self.loss_kwargs.get('tile_size')
        window = self.loss_kwargs.get('window_size')
        for eng, ix in zip(self.engines, self.groups):
            if tiles is not None and eng.objective_tiles != tuple(tiles):
                eng.set_objective_tiles(tiles)
            if window is not None and eng.splat_window != window:
                eng.set_splat_window(window)
            eng.set_windows([windows[b] for b in ix])
        if (prior_tau is not None or prior_gain is not None) and self._untransported is not None:
            self.prior = self._transported(self._untransported, tau=prior_tau, gain=prior_gain)

    def close(self):
        for eng in self.engines:
            eng.close()
        self.engines, self.engine = [], None

    def _params(self, lvl):
        kw = self.loss_kwargs
        return make_params(kw['alpha'], kw['beta'], kw['gamma'], kw['delta'], lvl, kw.get('scale_to_sensor_size_method', 'bilinear'),
                           kw.get('contrast_kind', 0), False, kw.get('correlation_kind', 'mse'))

    # -- one level: B BFGS solves in lockstep, with the reference's retries (solver.py:209-239) ---------------------------
    def _solve_level(self, k, starts):
        key = f'pyr_lvl_{k}'
        shape = starts[0].shape
        p = self._params(k)

        def fun_batch(X, mask):
            v, g, _ = self.engine.loss_grad(X.reshape((self.B,) + shape), p, active=mask)
            return v, g.reshape(self.B, -1)

        def launch(gi, X, mask):
            ix = self.groups[gi]
            self.engines[gi].loss_grad_async(X[ix].reshape((len(ix),) + shape), p, active=mask[ix])

        def collect(gi):
            v, g, _ = self.engines[gi].loss_grad_wait()
            return v, g.reshape(len(self.groups[gi]), -1)
        pipe = dict(groups=self.groups, launch=launch, collect=collect) if self.n_groups > 1 else {}
        gtol = self.theta_opt_solver_params['options']['gtol']
        extra = (self.theta_opt_solver_params.get('n_extra_attempts', {}) or {}).get(key, 0)
        x = np.stack([np.asarray(s, dtype=np.float64).reshape(-1) for s in starts])
        active = np.ones(self.B, bool)
        states = [None] * self.B
        on_device = self.bfgs_state == 'device' and x.shape[1] > _EXACT_UPDATE_MAX_N      # below: the host's bit-exact SciPy update
        if self.n_groups > 1:
            def fun_batch_groups(X, mask):              # (the limited host form over several contexts: every group launched, then collected)
                for gi in range(self.n_groups):
                    launch(gi, X, mask)
                vg = [collect(gi) for gi in range(self.n_groups)]
                v, g = np.empty(self.B), np.empty((self.B, X.shape[1]))
                for ix, (vi, gi_) in zip(self.groups, vg):
                    v[ix], g[ix] = vi, gi_
                return v, g
        stats = {}
        for attempt in range(1 + extra):
            for b in range(self.B):
                if active[b]:
                    self.callbacks[b].set_cur_pyr_lvl(k)
                    self.callbacks[b].reset_opt_iter()
            cbs = [(lambda r, cb=self.callbacks[b], sh=shape: cb(spo.OptimizeResult(x=np.asarray(r.x).reshape(sh), fun=r.fun)))
                   for b in range(self.B)]
            wolfe2 = self.theta_opt_solver_params.get('wolfe2_fallback', True)
            needs_x = None
            if on_device:      # a retry begins again from the last iterate with H = I, as a new LockstepBFGS does
                # (an EmptyCallback counts iterations and never looks at x: no download for it)
                plain = [type(self.callbacks[b]) is EmptyCallback for b in range(self.B)]
                cbs = [(self.callbacks[b] if plain[b] else cbs[b]) for b in range(self.B)]
                needs_x = [not q for q in plain]
            res = minimize_thetas(self.engine, x.reshape((self.B,) + shape), p, self.theta_opt_maxiters[key], gtol, hessian=self.hessian,
                                  history=self.history, bfgs_state=self.bfgs_state, callbacks=cbs, active=active,
                                  initial_scale=self.initial_scale, wolfe2_fallback=wolfe2, callback_needs_x=needs_x,
                                  fun_batch=fun_batch_groups if self.n_groups > 1 else fun_batch, pipeline=pipe, stats=stats)
            for b in range(self.B):
                if active[b]:
                    x[b], states[b] = res[b].x, _info(res[b])
            # another attempt from the last iterate for the windows that stopped without converging (solver.py:218-239)
            active = np.array([active[b] and (not states[b].success) and states[b].iter_num > 0 for b in range(self.B)])
            if not active.any():
                break
        self.n_batch_evals += stats['n_batch_evals']; self.n_window_evals += stats['n_window_evals']
        return [x[b].reshape(shape) for b in range(self.B)], states

    # -- handover (solver.py:302-347) ----------------------------------------------------------------------------------------
    def _handover(self, k, opt, ho_states, ho_weights):
        key, finer = f'pyr_lvl_{k}', f'pyr_lvl_{k - 1}'
        hs = self.handover_settings
        if self._first or not hs['use_handover']:
            return [opt[b] for b in range(self.B)]
        out = []
        solve = k in hs['solve_handover_for_levels']
        if solve:
            lvl = k - 1 if k > 0 else 0
            priors = [self.prior[b][finer if k > 0 else key] for b in range(self.B)]
            thetas = [self._upscale(opt[b], self.pyramid_bases[-k]) if k > 0 else opt[b] for b in range(self.B)]
            p = self._params(lvl)
            limits = tuple(hs.get('handover_limits', (0.0, 1.0)))
            a_cur = np.full(self.B, 0.5)
            hkey = f'pyr_lvl_{lvl}'
            for b in range(self.B):                 # a scalar L-BFGS-B per window; the other windows ride along at their weight
                def f(a, b=b):
                    aa = a_cur.copy(); aa[b] = float(np.asarray(a).reshape(-1)[0])
                    self.n_batch_evals += 1
                    gi = next(g for g, ix in enumerate(self.groups) if b in ix)      # the window's own context; its group rides along
                    ix = self.groups[gi]
                    v, dv = self.engines[gi].handover_loss_grad(aa[ix], np.stack([priors[i] for i in ix]),
                                                                np.stack([thetas[i] for i in ix]), p, want_grad=True)
                    k_loc = int(np.where(ix == b)[0][0])
                    return float(v[k_loc]), np.array([dv[k_loc]])
                r = spo.minimize(f, np.array([0.5]), jac=True, method=self.handover_opt_solver_params['method'],
                                 bounds=spo.Bounds([limits[0]], [limits[1]]),
                                 options={'gtol': self.handover_opt_solver_params['options']['gtol'],
                                          'maxiter': self.handover_opt_maxiters[hkey]})
                w = float(r.x[0])
                if hs['clip_solved_handover']:
                    w = float(np.clip(w, *hs['clip_solved_handover_limits']))
                a_cur[b] = w
                ho_states[b][key] = _info(r)
                ho_weights[b][key] = w
        for b in range(self.B):
            a = ho_weights[b][key] if solve else hs['alpha_handover']
            ho_weights[b][key] = a
            out.append(a * self.prior[b][key] + (1 - a) * opt[b])
        return out

    # -- solve (solver.py:197-267) -----------------------------------------------------------------------------------------------
    def solve(self):
        hs = self.handover_settings
        B, top = self.B, f'pyr_lvl_{self.n_pyr_lvls - 1}'
        if hs['use_downscaled_finest_priors']:
            for b in range(B):
                for k in range(1, self.n_pyr_lvls):
                    self.prior[b][f'pyr_lvl_{k}'] = self._downscale(self.prior[b][f'pyr_lvl_{k - 1}'], self.pyramid_bases[-(k - 1) - 1])
        for cb in self.callbacks:
            cb.reset()
        pre_opt = [self._pyramid_from_top(np.zeros((1, 1, 2))) for _ in range(B)]
        for b in range(B):
            pre_opt[b][top] = self.prior[b][top]
        opt = [dict() for _ in range(B)]
        ho_opt = [dict() for _ in range(B)]
        states = [dict() for _ in range(B)]
        ho_states = [dict() for _ in range(B)]
        ho_weights = [{f'pyr_lvl_{k}': 0.5 for k in range(self.n_pyr_lvls)} for _ in range(B)]
        for k in reversed(range(self.n_pyr_lvls)):
            key, nxt = f'pyr_lvl_{k}', f'pyr_lvl_{k - 1}'
            xs, sts = self._solve_level(k, [pre_opt[b][key] for b in range(B)])
            for b in range(B):
                opt[b][key], states[b][key] = xs[b], sts[b]
            hov = self._handover(k, [opt[b][key] for b in range(B)], ho_states, ho_weights)
            for b in range(B):
                ho_opt[b][key] = hov[b]
                if k != 0:
                    pre_opt[b][nxt] = self._upscale(hov[b], self.pyramid_bases[-k])
        results = []
        for b in range(B):
            results.append({'prior_theta_pyr': dict(self.prior[b]), 'pre_opt_theta_pyr': pre_opt[b], 'theta_opt_state_pyr': states[b],
                            'pre_handover_theta_pyr': opt[b], 'ho_opt_state_pyr': ho_states[b],
                            'final_handover_weight_pyr': ho_weights[b], 'final_theta_pyr': ho_opt[b]})
            self.prior[b] = dict(ho_opt[b])
        if self.prior_transport == 'advect':
            self._untransported = [dict(p) for p in ho_opt]
            self.prior = self._transported(self._untransported)
        self._first = False
        return results
