"""Time-and-phase alignment of two waveforms: what scri's frame fixing imports as `sxs.waveforms.alignment.align2d`
(scri/asymptotic_bondi_data/map_to_superrest_frame.py:9,979; map_to_abd_frame.py:15,217,253).

`sxs` (pinned ">=2022.4.0" by the pyproject.toml of scri) is a third-party package that is neither vendored by scri
nor in this image, so this is a restatement of its published algorithm, not a checked port -- parity with
the sxs implementation is UNPINNED; the tests pin the behaviour the reference relies on instead: the optimum (dt, dphi)
is the time translation and the turn about z whose BMSTransformation carries `wa` onto `wb`.

    wa'(t) = wa(t + dt) e^{i m dphi}      minimises      int_{t1}^{t2} sum_{lm} |wa'_{lm}(t) - wb_{lm}(t)|^2 dt
                                                          / int_{t1}^{t2} sum_{lm} |wb_{lm}(t)|^2 dt

A brute-force scan over (dt, dphi) seeds `scipy.optimize.least_squares`.  The scan costs one spline evaluation per dt:
the dphi dependence is  ||wa||^2 + ||wb||^2 - 2 Re sum_m e^{i m dphi} C_m(dt)  with  C_m = int sum_l wa_{lm}(t + dt) conj(wb_{lm}(t)) dt.

Two routes.  Without a context and with both waveforms in host memory everything above runs in numpy/scipy on the host.  With a
context (`ctx=`) or a device-resident waveform the arithmetic on waveform data runs on the GPU and the data stays there:

    cost(dt, dphi) = 1/2 [ N_a(dt) + N_b - 2 Re sum_m e^{i m dphi} C_m(dt) ] / N_b
    N_a(dt) = sum_i w_i sum_c |A_c(t_i + dt)|^2      C_m(dt) = sum_i w_i sum_{c: m_c = m} A_c(t_i + dt) conj(B_ic)      N_b = sum_i w_i sum_c |B_ic|^2

(t_i, w_i: window times of wb and their trapezoid weights; A_c: the not-a-knot cubic spline of wa's column over its whole axis; B_ic:
the rows of wb).  All dependence on dphi is in closed form once the MOMENTS N_a, C_m are known at a dt -- 1 + 2 n_m numbers -- and
their dt-derivatives are the same sums over the spline's derivatives, so one kernel (bms_align_moments) serves the scan (order 0 at
every offset of the grid, one call) and the refinement (orders 0..2 at one offset per step: exact gradient and Hessian of the cost for
a damped Newton step on the host).  The reported cost is summed directly (bms_align_residual): non-negative by construction and smooth
at a perfect match, where the moment form cancels to +-1e-17.  Only O(offsets x n_m) numbers cross the link.
"""
import numpy as np


def _window_rows(t, t1, t2):
    keep = (t >= t1) & (t <= t2)
    if keep.sum() < 4:
        raise ValueError(f"fewer than 4 samples of the fixed waveform lie in [{t1}, {t2}]")
    return keep


def _trapezoid_weights(t):
    w = np.zeros_like(t)
    w[:-1] += 0.5 * np.diff(t)
    w[1:] += 0.5 * np.diff(t)
    return w


def strain_of(abd):
    """The strain h = 2 sigma-bar of an AsymptoticBondiData object as align2d takes it: `abd.h`, except that a device-resident object
    yields a device-resident WaveformModes (one bms_mode_map launch: conjugation, the sign (-1)^m, the factor 2 and the cut to l >= 2)
    instead of sending sigma through the host."""
    if not getattr(abd, "is_device_resident", False):
        return abd.h
    from . import Inertial, WaveformModes, device_series
    from . import h as h_DataType

    sigma = abd.sigma
    perm, sign = device_series._bar_tables(0, abd._ell_max, sigma.spin_weight)
    w = WaveformModes(t=abd._time.copy(), frameType=Inertial, dataType=h_DataType, r_is_scaled_out=True, m_is_scaled_out=True, ctx=abd._ctx)
    w._host, w._dev = None, sigma._map(perm.size - 4, perm[4:], 2.0 * sign[4:], conj_a=True)
    w.ell_min, w.ell_max = 2, abd._ell_max
    return w


def _device_context(wa, wb, ctx):
    """the context of the device route, or None for the host route"""
    found = ctx
    for w in (wa, wb):
        if getattr(w, "is_device_resident", False):
            own = getattr(w, "_ctx", None)
            if own is None:
                from . import _lib

                own = _lib.default_context()
            if found is not None and own is not None and own is not found:
                raise ValueError("align2d: the waveforms and ctx= name two different contexts")
            found = own if found is None else found
    return found


def _cost_derivatives(M, ms, δϕ, normalization):
    """cost, gradient and Hessian in (dt, dphi) from the moments M[3, 1 + 2 n_m] of one offset (orders 0, 1, 2 along axis 0)"""
    e = np.exp(1j * ms * δϕ)
    C = M[:, 1::2] + 1j * M[:, 2::2]
    S = [np.sum(e * C[o]) for o in range(3)]
    f = 0.5 * (M[0, 0] + normalization - 2.0 * S[0].real) / normalization
    g = np.array([0.5 * (M[1, 0] - 2.0 * S[1].real), np.sum(ms * e * C[0]).imag]) / normalization
    H_tϕ = np.sum(ms * e * C[1]).imag
    H = np.array([[0.5 * (M[2, 0] - 2.0 * S[2].real), H_tϕ], [H_tϕ, np.sum(ms * ms * e * C[0]).real]]) / normalization
    return f, g, H


def _refine(moments, ms, normalization, x0, δt_lower, δt_upper, max_nfev=60, xtol=1e-12):
    """Bounded, damped Newton (Levenberg-style) iteration on (dt, dphi) from the seed x0.

    moments(δts, order) -> array [order + 1, len(δts), 1 + 2 len(ms)] (the layout of engine.align_moments): N_a and Re / Im of C_m at the
    offsets δts with their dt-derivatives.  dt is kept in [δt_lower, δt_upper]; dphi runs free (the caller wraps it).  A step solves
    (H + λ D) p = -g with the exact gradient and Hessian of the cost, D = diag|H| and λ raised until the matrix is positive definite and
    the cost does not increase; on a bound of dt with the gradient pointing outwards only dphi moves.  Returns (x, cost from the moment
    form, gradient, evaluations, status, message); status 1: the last step was below xtol (converged); 0: max_nfev
    reached; 2: a stall -- no damping up to 1e12 gave a step that does not increase the cost; -1: the moments are not finite.  Only
    status 1 counts as success."""
    ms = np.asarray(ms, dtype=float)
    x = np.array([min(max(float(x0[0]), δt_lower), δt_upper), float(x0[1])])

    def evaluate(x):
        return _cost_derivatives(np.asarray(moments(np.array([x[0]]), 2))[:, 0, :], ms, x[1], normalization)

    f, g, H = evaluate(x)
    nfev, λ = 1, 0.0
    status, message = 0, "the maximum number of evaluations was reached"
    floor = 64 * np.finfo(float).eps  # the moment form of the cost carries rounding of this size (in units of N_b)
    while nfev < max_nfev:
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(g))):
            status, message = -1, "the moments are not finite"
            break
        D = np.maximum(np.abs(np.diag(H)), 1e-300)
        on_bound = (x[0] <= δt_lower and g[0] > 0.0) or (x[0] >= δt_upper and g[0] < 0.0) or not (δt_upper > δt_lower)
        while True:
            a, b, d = H[0, 0] + λ * D[0], H[0, 1], H[1, 1] + λ * D[1]
            if on_bound:
                if d > 0.0:
                    p = np.array([0.0, -g[1] / d])
                    break
            elif a > 0.0 and a * d - b * b > 0.0:
                p = -np.array([d * g[0] - b * g[1], a * g[1] - b * g[0]]) / (a * d - b * b)
                break
            λ = max(4.0 * λ, 1e-3)
        x_new = np.array([min(max(x[0] + p[0], δt_lower), δt_upper), x[1] + p[1]])
        step = x_new - x
        if np.all(np.abs(step) <= xtol * np.maximum(1.0, np.abs(x))):
            status, message = 1, "the Newton step fell below xtol"
            break
        f_new, g_new, H_new = evaluate(x_new)
        nfev += 1
        if f_new <= f + floor:
            x, f, g, H = x_new, f_new, g_new, H_new
            λ = 0.0 if λ < 1e-6 else 0.1 * λ
        else:
            λ = max(10.0 * λ, 1e-3)
            if λ > 1e12:
                status, message = 2, "no step reduces the cost further"
                break
    return x, f, g, nfev, status, message


def _align2d_device(wa, wb, t1, t2, n_brute_force_δt, n_brute_force_δϕ, include_modes, ctx):
    """The device route of align2d: the same validation, offset grid and phase grid as the host route; moments from the GPU."""
    from scipy.optimize import OptimizeResult

    from . import device_series, engine

    ell_min, ell_max = max(wa.ell_min, wb.ell_min), min(wa.ell_max, wb.ell_max)
    LM = [(l, m) for l in range(ell_min, ell_max + 1) for m in range(-l, l + 1)]
    if include_modes is not None:
        wanted = {tuple(x) for x in include_modes}
        LM = [lm for lm in LM if lm in wanted]
    if not LM:
        raise ValueError("no common modes to align")
    col = lambda w: np.array([l * (l + 1) - w.ell_min**2 + m for l, m in LM])  # noqa: E731
    m_of = np.array([m for _, m in LM], dtype=float)
    ta, tb = np.asarray(wa.t, dtype=float), np.asarray(wb.t, dtype=float)
    if not (t1 < t2):
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is out of order")
    if t1 < tb[0] or t2 > tb[-1]:
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is not contained in wb, which spans ({tb[0]}, {tb[-1]})")
    δt_lower = max(t1 - t2, ta[0] - t1)
    δt_upper = min(t2 - t1, ta[-1] - t2)
    if not (δt_lower <= 0.0 <= δt_upper):
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is not contained in wa, which spans ({ta[0]}, {ta[-1]})")
    rows = _window_rows(tb, t1, t2)
    t = tb[rows]
    w = _trapezoid_weights(t)
    ms = np.unique(m_of)
    m_slot = np.searchsorted(ms, m_of)

    # ---- the two waveforms on the device: a resident one stays as it is (its .data is never read), a host one goes up once, its
    # common columns only.  The slopes come from the not-a-knot solve over the whole axis.
    resident = lambda x: getattr(x, "is_device_resident", False)  # noqa: E731
    if resident(wa):
        Y, col_a = wa._dev, col(wa)
        if (Y.shape[1] > 1 and Y.stride(1) != 1) or (Y.shape[0] > 1 and Y.stride(0) != Y.shape[1]):
            Y = Y.contiguous()  # (a padded or column-sliced view: the slopes come back dense, and the two share one row stride)
    else:
        Y, col_a = device_series.to_device(ctx, np.asarray(wa.data)[:, col(wa)]), np.arange(len(LM))
    first = int(np.argmax(rows))
    if resident(wb):
        B, col_b = wb._dev[first : first + t.size], col(wb)
    else:
        B, col_b = device_series.to_device(ctx, np.asarray(wb.data)[rows][:, col(wb)]), np.arange(len(LM))
    S = engine.knot_slopes(ta, Y, ctx=ctx)
    series = (ta, Y, S, col_a, t, w, B, col_b)

    def moments(δts, order):
        return engine.align_moments(*series, m_slot, ms.size, δts, order, ctx=ctx)

    normalization = engine.align_residual(*series, m_of, 0.0, 0.0, ctx=ctx)[1]
    if not normalization > 0.0:
        raise ValueError("wb vanishes on the window: nothing to align to")

    # ---- brute force: one order-0 call for every dt, the (2 l_max + 1)-term sum over dphi on the small result
    in_a = ((ta >= t1 + δt_lower) & (ta <= t2 + δt_upper)).sum()
    if n_brute_force_δt is None:
        n_brute_force_δt = int(max(in_a, rows.sum()))
    if n_brute_force_δϕ is None:
        n_brute_force_δϕ = 2 * ell_max + 1
    δts = np.linspace(δt_lower, δt_upper, max(int(n_brute_force_δt), 1)) if δt_upper > δt_lower else np.array([0.0])
    if not np.any(δts == 0.0):
        δts = np.sort(np.append(δts, 0.0))
    δϕs = np.linspace(0.0, 2 * np.pi, max(int(n_brute_force_δϕ), 1), endpoint=False)
    phases = np.exp(1j * np.outer(δϕs, ms))  # [n_dphi, n_m]
    M = moments(δts, 0)[0]
    costs = M[:, :1] + normalization - 2.0 * ((M[:, 1::2] + 1j * M[:, 2::2]) @ phases.T).real  # [n_dt, n_dphi]
    k_t, k_ϕ = np.unravel_index(int(np.argmin(costs)), costs.shape)

    # ---- refine.  dphi is periodic: it runs free around the seed and is wrapped afterwards
    x, _, grad, nfev, status, message = _refine(moments, ms, normalization, (δts[k_t], δϕs[k_ϕ]), δt_lower, δt_upper)
    x[1] = np.mod(x[1], 2 * np.pi)
    residual, _ = engine.align_residual(*series, m_of, x[0], x[1], ctx=ctx)
    optimum = OptimizeResult(x=x, cost=0.5 * residual / normalization, grad=grad, nfev=nfev, success=status == 1, status=status, message=message)

    all_m = np.array([m for l in range(wa.ell_min, wa.ell_max + 1) for m in range(-l, l + 1)], dtype=float)
    turn = np.exp(1j * all_m * x[1])
    if resident(wa):  # one launch into a new device array; the result stays resident
        series_dev = device_series.DeviceModesTimeSeries(wa._dev, ta, 0, wa.ell_min, wa.ell_max, ctx=ctx)
        wa_prime = wa.copy_without_data()
        wa_prime.frame = np.array(wa.frame, copy=True)
        wa_prime._host, wa_prime._dev = None, series_dev._map(all_m.size, np.arange(all_m.size, dtype=np.int32), turn)
    else:
        wa_prime = wa.copy()
        wa_prime.data = np.asarray(wa.data) * turn[None, :]
    wa_prime.t = ta - x[0]
    return optimum.cost, wa_prime, optimum


def align2d(wa, wb, t1, t2, n_brute_force_δt=None, n_brute_force_δϕ=None, include_modes=None, nprocs=None, ctx=None):
    """Optimal time offset and turn about z to apply to `wa` so that it matches `wb` on [t1, t2].

    wa, wb: WaveformModes-like objects (.t, .data [n, modes], .ell_min, .ell_max, .LM); include_modes: optional list of
    (l, m) pairs the cost is restricted to; nprocs is accepted for call compatibility (the scan is vectorised instead).

    Returns (error, wa_prime, optimum): error = optimum.cost = half the normalised squared L2 distance at the optimum,
    wa_prime = `wa` on the times wa.t - dt with every mode multiplied by e^{i m dphi}, optimum = the
    scipy.optimize.OptimizeResult with optimum.x = [dt, dphi].

    With `ctx` (an engine context) or a device-resident waveform the scan, the refinement and the cost run on the GPU (module
    docstring): neither input loses its residency, `wa_prime` of a resident `wa` is resident, and `optimum` carries x, cost, grad,
    nfev, success (status 1: the Newton step fell below its tolerance; a stall or an exhausted budget is not success), status and message -- `fun` and `jac` are absent on this route: they are window x modes in size and would have to
    cross the link.  Without either the host route below runs, unchanged."""
    device_ctx = _device_context(wa, wb, ctx)
    if device_ctx is not None:
        return _align2d_device(wa, wb, t1, t2, n_brute_force_δt, n_brute_force_δϕ, include_modes, device_ctx)
    from scipy.interpolate import CubicSpline
    from scipy.optimize import least_squares

    ell_min, ell_max = max(wa.ell_min, wb.ell_min), min(wa.ell_max, wb.ell_max)
    LM = [(l, m) for l in range(ell_min, ell_max + 1) for m in range(-l, l + 1)]
    if include_modes is not None:
        wanted = {tuple(x) for x in include_modes}
        LM = [lm for lm in LM if lm in wanted]
    if not LM:
        raise ValueError("no common modes to align")
    col = lambda w: np.array([l * (l + 1) - w.ell_min**2 + m for l, m in LM])  # noqa: E731
    m_of = np.array([m for _, m in LM], dtype=float)
    ta, tb = np.asarray(wa.t, dtype=float), np.asarray(wb.t, dtype=float)
    if not (t1 < t2):
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is out of order")
    if t1 < tb[0] or t2 > tb[-1]:
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is not contained in wb, which spans ({tb[0]}, {tb[-1]})")
    δt_lower = max(t1 - t2, ta[0] - t1)
    δt_upper = min(t2 - t1, ta[-1] - t2)
    if not (δt_lower <= 0.0 <= δt_upper):
        raise ValueError(f"(t1, t2) = ({t1}, {t2}) is not contained in wa, which spans ({ta[0]}, {ta[-1]})")

    rows = _window_rows(tb, t1, t2)
    t = tb[rows]
    B = np.asarray(wb.data)[rows][:, col(wb)]
    a_of = CubicSpline(ta, np.asarray(wa.data)[:, col(wa)])
    w = _trapezoid_weights(t)
    normalization = w @ np.sum(np.abs(B) ** 2, axis=1)
    if not normalization > 0.0:
        raise ValueError("wb vanishes on the window: nothing to align to")
    ms = np.unique(m_of)
    m_slot = np.searchsorted(ms, m_of)

    # residual vector whose squared length is the normalised squared distance (trapezoid weights folded in): the same
    # `cost` as a single scalar residual, but smooth at a perfect match
    root_w = np.sqrt(w / normalization)[:, None]

    def residual(x):
        A = a_of(t + x[0]) * np.exp(1j * m_of * x[1])
        return np.ascontiguousarray((A - B) * root_w).view(float).ravel()

    # ---- brute force: every dt costs one spline evaluation, every dphi a (2 l_max + 1)-term sum
    in_a = ((ta >= t1 + δt_lower) & (ta <= t2 + δt_upper)).sum()
    if n_brute_force_δt is None:
        n_brute_force_δt = int(max(in_a, rows.sum()))
    if n_brute_force_δϕ is None:
        n_brute_force_δϕ = 2 * ell_max + 1
    δts = np.linspace(δt_lower, δt_upper, max(int(n_brute_force_δt), 1)) if δt_upper > δt_lower else np.array([0.0])
    if not np.any(δts == 0.0):
        δts = np.sort(np.append(δts, 0.0))
    δϕs = np.linspace(0.0, 2 * np.pi, max(int(n_brute_force_δϕ), 1), endpoint=False)
    phases = np.exp(1j * np.outer(δϕs, ms))  # [n_dphi, n_m]
    best = (np.inf, 0.0, 0.0)
    for δt in δts:
        A = a_of(t + δt)
        norm_a = w @ np.sum(np.abs(A) ** 2, axis=1)
        cross = w @ (A * np.conj(B))  # per mode
        C = np.zeros(ms.size, dtype=complex)
        np.add.at(C, m_slot, cross)
        costs = norm_a + normalization - 2.0 * (phases @ C).real
        k = int(np.argmin(costs))
        if costs[k] < best[0]:
            best = (costs[k], δt, δϕs[k])

    # ---- refine.  dphi is periodic: let it run free around the seed and wrap afterwards
    x0 = np.array([best[1], best[2]])
    lo = np.array([δt_lower, x0[1] - np.pi])
    hi = np.array([δt_upper, x0[1] + np.pi])
    if hi[0] <= lo[0]:
        lo[0], hi[0] = lo[0] - 1e-12, hi[0] + 1e-12
    optimum = least_squares(residual, np.clip(x0, lo, hi), bounds=(lo, hi), xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=50000)
    optimum.x[1] = np.mod(optimum.x[1], 2 * np.pi)

    wa_prime = wa.copy()
    all_m = np.array([m for l in range(wa.ell_min, wa.ell_max + 1) for m in range(-l, l + 1)], dtype=float)
    wa_prime.data = np.asarray(wa.data) * np.exp(1j * all_m * optimum.x[1])[None, :]
    wa_prime.t = ta - optimum.x[0]
    return optimum.cost, wa_prime, optimum
