"""The float64 reference of the natural-gradient step with momentum (SPRING: Goldshlager, Abrahamsen, Lin 2024) — a plain helper
module beside sr_reference.py, whose definitions (X_b, T_b, y_b, lambda_b for b in {a, phi}) it uses.

With the previous step phi_prev and 0 <= mu < 1 the step regularises towards mu phi_prev instead of 0:

    phi = argmin_p  sum_b |X_b p - y_b|^2 / lambda_b + |p - mu phi_prev|^2
        = mu phi_prev + sum_b X_b^T (T_b + lambda_b I)^-1 (y_b - mu X_b phi_prev)

(the two blocks decouple: no parameter moves both log|psi| and the phase).  X_b phi_prev = sqrt(w) o (u_b - w^T u_b) with the
Jacobian-vector products u_a = A phi_prev, u_phi = B phi_prev — ``naqs_net_sr_jvp``.

* ``jvp64``                 (A v, B v);
* ``jvp_err``               max_i |u_i - (J v)_i| / (|J| |v|)_i, the measure of the kernels' products;
* ``spring_direction``      the step above in float64 numpy (dense solves); mu = 0 is ``sr_reference.direction``;
* ``stationarity``          the residual of the minimisation's normal equations, relative to the step;
* ``spring_direction_f32``  the same step as a float32 network on the CPU takes it, built as ``sr_reference.direction_f32`` is:
                            float32 Jacobian rows, float64 products and solves, float32 seeds, a float32 backward, and phi_prev
                            rounded to float32 — the yardstick of the kernels' step.
"""
import numpy as np

import grad_reference as gr
import sr_reference as sr


def jvp64(A, B, v):
    v = np.asarray(v, np.float64)
    return A @ v, B @ v


def jvp_err(u, J, v):
    """max over the rows of |u_i - (J v)_i| / (|J| |v|)_i (rows whose scale is zero must be zero)."""
    v = np.asarray(v, np.float64)
    scale = np.abs(J) @ np.abs(v)
    diff = np.abs(np.asarray(u, np.float64) - J @ v)
    assert np.all(diff[scale == 0] == 0)
    return float(np.max(diff / np.where(scale > 0, scale, 1.0)))


def _blocks(A, B, w, g, diag_shift):
    for J, col in ((A, 0), (B, 1)):
        T, y, X = sr.system(J, w, np.asarray(g)[:, col], diag_shift)
        yield T, y, X, diag_shift * (X * X).sum() / len(w)         # (T is T_b + lambda_b I; lambda_b = diag_shift tr T_b / M)


def spring_direction(A, B, w, g, diag_shift, mu, phi_prev):
    """phi float64 [N_p]; ``phi_prev`` None counts as 0."""
    prev = np.zeros(A.shape[1]) if phi_prev is None else np.asarray(phi_prev, np.float64)
    out = mu * prev
    for T, y, X, _ in _blocks(A, B, w, g, diag_shift):
        out = out + X.T @ np.linalg.solve(T, y - mu * (X @ prev))
    return out


def stationarity(A, B, w, g, diag_shift, mu, phi_prev, phi):
    """max |sum_b X_b^T (X_b psi - r_b) / lambda_b + psi| / max |psi|, psi = phi - mu phi_prev, r_b = y_b - mu X_b phi_prev."""
    prev = np.asarray(phi_prev, np.float64)
    psi = np.asarray(phi, np.float64) - mu * prev
    res = psi.copy()
    for _, y, X, lam in _blocks(A, B, w, g, diag_shift):
        res = res + X.T @ (X @ psi - (y - mu * (X @ prev))) / lam
    return float(np.abs(res).max() / np.abs(psi).max())


def spring_direction_f32(w32, states, A32, B32, w, g, diag_shift, mu, phi_prev):
    """The float32-CPU pipeline: ``sr_reference.direction_f32`` with the right-hand sides y - mu X32 phi_prev (phi_prev rounded to
    float32, the product in float64) and mu phi_prev added to the float32 backward's result in float32."""
    prev = np.asarray(phi_prev, np.float64).astype(np.float32)
    sw = np.sqrt(w)
    seeds = []
    for T, y, X, _ in _blocks(A32, B32, w, g, diag_shift):
        x = np.linalg.solve(T, y - mu * (X @ prev.astype(np.float64)))
        seeds.append(sw * x - w * (sw @ x))
    grads = gr.grad_f64(w32, states, np.stack(seeds, -1).astype(np.float32))
    d = np.concatenate([grads[n].reshape(-1) for n, _ in w32.model.named_parameters()]).astype(np.float32)
    return (np.float32(mu) * prev + d).astype(np.float64)
