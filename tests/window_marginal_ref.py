"""A numpy restatement of mh_icp_window_marginalise, written from the contract in include/mimosa_hip.h and not from
mimosa_amd/csrc/window_device.hpp: every term that touches pose 0 of the window, evaluated at the poses given, accumulated
into dense blocks and eliminated with numpy.linalg.solve.  Transport of the linear factors is tests/window_lin_ref.py's, the
between terms are tests/window_edge_ref.py's.  Shared by tests/test_icp_window_marginal_cpu.py and
tests/test_gpu_icp_window_marginal.py.

icp0: (H, b, f) of the oldest factor at pose 0 after the 4-DoF projection and the degeneracy quirk, or None (empty factor).
Returns a dict: H, b, f (the model f + 2 b^T x + x^T H x in the tangent of pose 1), valid, n_ties, and the accumulated blocks
A00, A10, A11, g0, g1, c — the uncancelled scales a comparison is relative to."""
import numpy as np

import window_edge_ref as edge_ref
import window_lin_ref as lin_ref


def marginal(poses, icp0, has_Z1, Z1, Wb, prior, damping, linear, edges):
    A00, A10, A11 = np.zeros((6, 6)), np.zeros((6, 6)), np.zeros((6, 6))
    g0, g1, c = np.zeros(6), np.zeros(6), 0.0
    if icp0 is not None:
        A00 += np.asarray(icp0[0], float).reshape(6, 6)
        g0 += np.asarray(icp0[1], float)
        c += float(icp0[2])
    for l in linear:
        if l["pose"] != 0:
            continue
        H, b, f = lin_ref.transport(np.asarray(l["H"], float).reshape(6, 6), np.asarray(l["b"], float), float(l["f"]), l["at"], poses[0])
        A00 += H
        g0 += b
        c += f
    ties = [dict(a=0, b=1, Z=Z1, info=np.diag(Wb))] if has_Z1 else []
    for e in edges:
        assert not (e["a"] == 0 and e["b"] > 1), "only the separator {1}"
        if (e["a"], e["b"]) == (0, 1):
            ties.append(e)
    for e in ties:
        _, _, Baa, Eba, ga, gb, cz = edge_ref.edge_terms(poses[0], poses[1], e["Z"], e["info"])
        A00 += Baa
        A10 += Eba
        A11 += np.asarray(e["info"], float).reshape(6, 6)
        g0 += ga
        g1 += gb
        c += cz
    A00 = A00 + np.diag(prior) + damping * np.eye(6)
    out = dict(A00=A00, A10=A10, A11=A11, g0=g0, g1=g1, c=c, n_ties=len(ties))
    try:
        np.linalg.cholesky(A00)
    except np.linalg.LinAlgError:
        return dict(out, H=np.zeros((6, 6)), b=np.zeros(6), f=0.0, valid=0)
    X = np.linalg.solve(A00, np.column_stack([A10.T, g0]))
    H = A11 - A10 @ X[:, :6]
    return dict(out, H=(H + H.T) / 2.0, b=g1 - A10 @ X[:, 6], f=c - g0 @ X[:, 6], valid=1)


def deviation(got, want):
    """(H, b, f): Frobenius norm of H_m - H_ref relative to ||A11'||_F, b_m relative to ||g1'||, f_m relative to c — the
    uncancelled scales.  Without a tie A11' and g1' are zero and so must the differences be: they are then reported as they are."""
    nH, nb, nf = np.linalg.norm(want["A11"]), np.linalg.norm(want["g1"]), abs(want["c"])
    dH = np.linalg.norm(np.asarray(got["H"], float).reshape(6, 6) - want["H"])
    db = np.linalg.norm(np.asarray(got["b"], float) - want["b"])
    df = abs(float(got["f"]) - want["f"])
    return dH / nH if nH > 0 else dH, db / nb if nb > 0 else db, df / nf if nf > 0 else df


def as_linear(m, T1, pose=0):
    """the marginal as a linear factor (tests/window_lin_ref.py's dicts) on `pose` of the window without its oldest pose"""
    return dict(pose=int(pose), at=T1, H=np.asarray(m["H"], float).reshape(6, 6), b=np.asarray(m["b"], float), f=float(m["f"]))
