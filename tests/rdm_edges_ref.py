"""numpy complex128 restatement of the two-site reduced density matrix of a bond from the BP environment (the reference's
reduced_density_matrix(cache, [u, v]; alg = "bp"), src/rdm.jl:52-73, for adjacent u, v: the Steiner tree is the bond itself), sharing no code with
the package: what tests/test_rdm_edges_ref_cpu.py pins against the oracle's region contraction and against exact state vectors, and what
tests/test_gpu_rdm_edges.py compares the device against.

Conventions (those of the package and of the oracle): the tensor of v has axes (site, leg to each neighbour in ascending vertex position); a message
(src, dst) is chi x chi with axes (ket, bra); `nbrs[v]` lists the neighbours of v in that order.

  env        E_u[s, a, s', a'] = sum_rest (psi_u x_{k != v} m_{k -> u})[s, a, rest] conj(psi_u[s', a', rest])
  rdm_edge   rho[s_u, s_v ; s_u', s_v'] = sum_{a, a'} E_u[s_u, a, s_u', a'] E_v[s_v, a, s_v', a'], un-normalised, as a (d_u d_v) x (d_u d_v) matrix with the
             FIRST vertex most significant (row = s_v + d_v s_u): tr(np.kron(O_u, O_v) @ rho) / tr(rho) is <O_u O_v>"""
import numpy as np


def env(tensors, messages, nbrs, u, v):
    psi = np.asarray(tensors[u], dtype=np.complex128)
    t = psi
    for j, k in enumerate(nbrs[u]):
        if k == v:
            continue
        m = np.asarray(messages[(k, u)], dtype=np.complex128)
        t = np.moveaxis(np.tensordot(t, m, axes=([1 + j], [0])), -1, 1 + j)       # the ket leg through m[ket, bra]
    jv = 1 + nbrs[u].index(v)
    rest = [a for a in range(1, psi.ndim) if a != jv]
    return np.tensordot(t, psi.conj(), axes=(rest, rest))                          # [s, a, s', a']


def rdm_edge(tensors, messages, nbrs, u, v):
    eu, ev = env(tensors, messages, nbrs, u, v), env(tensors, messages, nbrs, v, u)
    r = np.einsum("saSb,taTb->stST", eu, ev)
    du, dv = r.shape[0], r.shape[1]
    return r.reshape(du * dv, du * dv)


def expect_edge(tensors, messages, nbrs, u, v, op_u, op_v):
    rho = rdm_edge(tensors, messages, nbrs, u, v)
    return complex(np.trace(np.kron(op_u, op_v) @ rho) / np.trace(rho))
