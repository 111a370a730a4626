"""Mesh-free joint tables: what the posed joints of a model need when no vertex is formed.

``SMAL.__call__`` regresses the posed joints from the posed vertices (reference smal_model/smal_torch.py:340-351).  For the two
kinds of model this project ships no vertex is needed:

* static-joint models (``static_joints``): ``joints = J_transformed``, the translation column of the kinematic chain;
* regressor models without pose blend shapes: with ``A_k`` the relative skinning transform of bone ``k``,

      joints[j] = sum_v Jreg[j,v] sum_k w[v,k] A_k [v_shaped[v]; 1] = sum_k A_k m[j,k],
      m[j,k]    = sum_v Jreg[j,v] w[v,k] [v_shaped[v]; 1]            (a moment in R^4, a function of the shape only),

  and ``v_shaped`` is affine in the shape coefficients, so ``m = M0 + sum_b beta_b MB_b`` (the fourth component, the weight sum,
  does not move with the shape) and the rest joints are ``J_rest = J0 + sum_b beta_b JB_b``.

``JointTables.from_tables`` builds these tables once per model in float64 on the host.  Only (joint, bone) pairs with a non-zero
weight product are kept (STICK: 114 pairs, at most 4 per joint), listed twice: by joint (forward, the shape gradient) and by bone
(the gather of the gradient on ``A_k`` without atomics).  Nothing here touches a GPU; ``smilify_amd/csrc/joints.hip`` reads the
tables through ``engine.DeviceJointTables``.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import MAX_JOINTS  # the skin table's 8-bit bone ids
from .model_io import MAX_BONES_PER_VERTEX, SmilModelTables


@dataclass
class JointTables:
    """Float64 host tables of one model (see the module header).  ``P`` pairs; ``P == 0`` for a static-joint model."""

    J: int
    nB: int
    static_joints: bool
    parents: np.ndarray      # (J,) i32
    depth: np.ndarray        # (J,) i32
    child_ptr: np.ndarray    # (J+1,) i32  children of every joint, ascending (the reverse chain walk gathers from them)
    child: np.ndarray        # (J-1,) i32
    J0: np.ndarray           # (J,3)    rest joints of the template (J_static for a static-joint model)
    JB: np.ndarray           # (nB,J,3) their shape directions (zeros for a static-joint model)
    pair_ptr: np.ndarray     # (J+1,) i32  pairs by JOINT: pairs pair_ptr[j] .. pair_ptr[j+1] belong to joint j, bones ascending
    pair_bone: np.ndarray    # (P,) i32
    M0: np.ndarray           # (P,4)    moment of the template, fourth component = sum_v Jreg[j,v] w[v,k]
    MB: np.ndarray           # (P,nB,3) its shape directions
    bpair_ptr: np.ndarray    # (J+1,) i32  the same pairs by BONE: entries bpair_ptr[k] .. bpair_ptr[k+1] belong to bone k, joints ascending
    bpair_joint: np.ndarray  # (P,) i32
    bpair_index: np.ndarray  # (P,) i32  index of the entry's pair in the by-joint order (into M0 / MB)
    rowsum: np.ndarray       # (J,)     sum_v Jreg[j,v]: the factor of a translation added BEFORE the regression (1 +- 1e-7, not 1)

    @property
    def P(self) -> int:
        return int(self.pair_bone.shape[0])

    @property
    def max_depth(self) -> int:
        return int(self.depth.max())

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def from_tables(t: SmilModelTables, del_v=None, v_template=None) -> "JointTables":
        if t.posedirs is not None:
            raise NotImplementedError(
                "JointTables: the model has pose blend shapes (posedirs): they move the vertices with every frame's pose, so no "
                "pose-independent moment exists; use SMAL.__call__")
        if del_v is not None:
            raise NotImplementedError("JointTables: per-frame vertex offsets (del_v) change the moments per frame; use SMAL.__call__")
        if v_template is not None:
            raise NotImplementedError("JointTables: a v_template override changes the moments of the model; build the tables from a "
                                      "model that holds that template, or use SMAL.__call__")
        J, V, nB = t.J, t.V, t.nB
        if not 1 <= J <= MAX_JOINTS:
            raise ValueError(f"JointTables: J={J} outside 1..{MAX_JOINTS}")
        parents = np.ascontiguousarray(t.parents, np.int32)
        depth = np.ascontiguousarray(t.depth, np.int32)
        order = np.argsort(parents[1:], kind="stable").astype(np.int32) + 1  # children by parent, ascending within a parent
        child_ptr = np.zeros(J + 1, np.int32)
        np.add.at(child_ptr, parents[1:] + 1, 1)
        child_ptr = np.cumsum(child_ptr).astype(np.int32)
        z_i = np.zeros(0, np.int32)
        if t.static_joints:
            return JointTables(J=J, nB=nB, static_joints=True, parents=parents, depth=depth, child_ptr=child_ptr, child=order,
                               J0=np.asarray(t.J_static, np.float64).copy(), JB=np.zeros((nB, J, 3)), pair_ptr=np.zeros(J + 1, np.int32),
                               pair_bone=z_i, M0=np.zeros((0, 4)), MB=np.zeros((0, nB, 3)), bpair_ptr=np.zeros(J + 1, np.int32),
                               bpair_joint=z_i, bpair_index=z_i, rowsum=np.ones(J))
        vt = np.asarray(t.v_template, np.float64)
        sd = np.asarray(t.shapedirs, np.float64).reshape(nB, V, 3)
        W = np.zeros((V, J))
        np.add.at(W, (np.repeat(np.arange(V), MAX_BONES_PER_VERTEX), t.skin_idx.reshape(-1)), t.skin_w.reshape(-1).astype(np.float64))
        J0, JB, rowsum = np.zeros((J, 3)), np.zeros((nB, J, 3)), np.zeros(J)
        pair_ptr = np.zeros(J + 1, np.int32)
        bones, M0, MB = [], [], []
        for j in range(J):
            s, e = int(t.jreg_rowptr[j]), int(t.jreg_rowptr[j + 1])
            vs, r = t.jreg_col[s:e], t.jreg_val[s:e].astype(np.float64)
            J0[j] = r @ vt[vs]
            JB[:, j] = np.einsum("v,bvc->bc", r, sd[:, vs])
            rowsum[j] = r.sum()
            coef = r[:, None] * W[vs]  # (n,J): Jreg[j,v] w[v,k]
            for k in np.nonzero((coef != 0).any(0))[0]:
                c = coef[:, k]
                bones.append(int(k))
                M0.append(np.concatenate([c @ vt[vs], [c.sum()]]))
                MB.append(np.einsum("v,bvc->bc", c, sd[:, vs]))
            pair_ptr[j + 1] = len(bones)
        P = len(bones)
        pair_bone = np.asarray(bones, np.int32).reshape(P)
        pair_joint = np.repeat(np.arange(J, dtype=np.int32), np.diff(pair_ptr))
        by_bone = np.argsort(pair_bone, kind="stable").astype(np.int32)
        bpair_ptr = np.zeros(J + 1, np.int32)
        np.add.at(bpair_ptr, pair_bone + 1, 1)
        return JointTables(J=J, nB=nB, static_joints=False, parents=parents, depth=depth, child_ptr=child_ptr, child=order, J0=J0, JB=JB,
                           pair_ptr=pair_ptr, pair_bone=pair_bone, M0=np.asarray(M0, np.float64).reshape(P, 4),
                           MB=np.asarray(MB, np.float64).reshape(P, nB, 3), bpair_ptr=np.cumsum(bpair_ptr).astype(np.int32),
                           bpair_joint=pair_joint[by_bone], bpair_index=by_bone, rowsum=rowsum)

    # ------------------------------------------------------------------------------------------
    # float64 numpy evaluation (tests, and the statement of what the kernels compute)
    # ------------------------------------------------------------------------------------------
    def _beta(self, beta) -> np.ndarray:
        b = np.atleast_2d(np.asarray(beta, np.float64))
        if b.shape[1] > self.nB:
            raise ValueError(f"beta has {b.shape[1]} columns but the model has {self.nB} shape directions")
        return b

    def rest_joints(self, beta) -> np.ndarray:
        """(S,J,3) for beta (S,nB_used) (or (nB_used,): S = 1)."""
        b = self._beta(beta)
        return self.J0[None] + np.einsum("sb,bjc->sjc", b, self.JB[: b.shape[1]])

    def moments(self, beta) -> np.ndarray:
        """(S,P,4)."""
        b = self._beta(beta)
        m = np.repeat(self.M0[None], b.shape[0], 0)
        m[:, :, :3] += np.einsum("sb,pbc->spc", b, self.MB[:, : b.shape[1]])
        return m

    def joints_from_transforms(self, A, beta, trans: Optional[np.ndarray] = None, trans_after_joints: bool = True) -> np.ndarray:
        """Posed joints (B,J,3) from the relative skinning transforms A (B,J,3,4) of the chain: ``sum_k A_k m[j,k]`` for a regressor
        model, ``A_j [J_rest[j]; 1]`` (= J_transformed) for a static-joint one.  ``trans`` (B,3) is added to the joints
        (``trans_after_joints``, the fitter's convention) or, as ``SMAL.__call__`` does, to the vertices before the regression: times
        ``rowsum`` for a regressor model, not at all for a static-joint one (smal_torch.py:343-346)."""
        A = np.asarray(A, np.float64)
        B = A.shape[0]
        if self.static_joints:
            Jr = np.broadcast_to(self.rest_joints(beta), (B, self.J, 3))
            out = np.einsum("bjrc,bjc->bjr", A[..., :3], Jr) + A[..., 3]
            factor = np.ones(self.J) if trans_after_joints else np.zeros(self.J)
        else:
            m = np.broadcast_to(self.moments(beta), (B, self.P, 4))
            terms = np.einsum("bprc,bpc->bpr", A[:, self.pair_bone], m)
            out = np.zeros((B, self.J, 3))
            for j in range(self.J):
                out[:, j] = terms[:, self.pair_ptr[j]:self.pair_ptr[j + 1]].sum(1)
            factor = np.ones(self.J) if trans_after_joints else self.rowsum
        if trans is not None:
            out = out + factor[None, :, None] * np.asarray(trans, np.float64)[:, None, :]
        return out
