"""numpy complex128 restatement of the two-site reduced density matrices of the two ENDS of a path from the BP environment (the reference's
reduced_density_matrix(cache, [u, w]; alg = "bp"), src/rdm.jl:52-73, where the Steiner tree of u and w is a path p_0 = u, p_1, .., p_n = w), sharing no code
with the package: what tests/test_path_rdm_ref_cpu.py pins against the oracle's region contraction and against exact state vectors, and what
tests/test_gpu_path_rdm.py compares the device against.  Conventions as in tests/rdm_edges_ref.py, whose `env` is E below.

  L_0[s, a, s', a']    = E_{p_0 -> p_1}[s, a, s', a']                                                 a: the bond p_0 - p_1
  transfer             T_k[a, b, a', b'] = sum_{s, rest} (psi_{p_k} x_{legs off the path} m)[s, a, b, rest] conj(psi_{p_k}[s, a', b', rest])
                       a: the bond from p_{k-1}, b: the bond to p_{k+1}
  L_k[s, b, s', b']    = sum_{a, a'} L_{k-1}[s, a, s', a'] T_k[a, b, a', b']                          k = 1 .. n - 1
  rho_{u, p_k}         = sum_{a, a'} L_{k-1}[s_u, a, s_u', a'] E_{p_k -> p_{k-1}}[s_w, a, s_w', a']   k = 1 .. n
un-normalised, as a (d_u d_w) x (d_u d_w) matrix with the FIRST vertex most significant.  The path must be induced: the region contraction it restates sums over
every bond between region vertices, and a chord is such a bond."""
import numpy as np

from rdm_edges_ref import env


def transfer(tensors, messages, nbrs, v, prev, nxt):
    psi = np.asarray(tensors[v], dtype=np.complex128)
    t = psi
    for j, k in enumerate(nbrs[v]):
        if k == prev or k == nxt:
            continue
        m = np.asarray(messages[(k, v)], dtype=np.complex128)
        t = np.moveaxis(np.tensordot(t, m, axes=([1 + j], [0])), -1, 1 + j)
    ja, jb = 1 + nbrs[v].index(prev), 1 + nbrs[v].index(nxt)
    rest = [a for a in range(psi.ndim) if a not in (ja, jb)]                     # the site index and every leg off the path
    out = np.tensordot(t, psi.conj(), axes=(rest, rest))                         # kept axes in tensor order on either side
    if ja > jb:
        out = out.transpose(1, 0, 3, 2)
    return out                                                                   # [a, b, a', b']


def is_induced_path(nbrs, path):
    path = list(path)
    if len(path) < 2 or len(set(path)) != len(path):
        return False
    return all((path[q] in nbrs[path[k]]) == (q == k + 1) for k in range(len(path)) for q in range(k + 1, len(path)))


def path_rdms(tensors, messages, nbrs, path):
    """[rho_{p_0, p_k} for k = 1 .. len(path) - 1]"""
    assert is_induced_path(nbrs, path), path
    L = env(tensors, messages, nbrs, path[0], path[1])
    out = []
    for k in range(1, len(path)):
        e = env(tensors, messages, nbrs, path[k], path[k - 1])
        r = np.einsum("saSb,taTb->stST", L, e)
        du, dw = r.shape[0], r.shape[1]
        out.append(r.reshape(du * dw, du * dw))
        if k + 1 < len(path):
            L = np.einsum("saSc,abcd->sbSd", L, transfer(tensors, messages, nbrs, path[k], path[k - 1], path[k + 1]))
    return out


def expect_pair(rho, op_u, op_w):
    return complex(np.trace(np.kron(op_u, op_w) @ rho) / np.trace(rho))
