"""`BatchVerifier` (halo2_proofs/src/plonk/verifier/batch.rs): many proofs of one verifying key checked with ONE `MSM::eval`.

Each proof is read up to its Guard (halo2_amd/verifier.py `_verify_guard`) and kept as a `Claim`: the x-keyed point terms, the w
and u scalars, the G_0 constant and the (neg_c, u_0 .. u_{k-1}) of its s vector -- a few hundred host scalars, no n-element
device vector.  `combine_claims` weights the claims with independent random nonzero factors r_b and sums them: the point terms,
w and u on the host (the x-keyed sign rule of msm.rs:63-84), the g part as ONE n-element vector

    g_scalars = sum_b r_b * neg_c_b * compute_s(u_b, 1)  +  (sum_b r_b * (-v_b)) at index 0

built by one h2_ipa_s_combine_device launch.  The batch then costs one commit over g and one small generic multiexp, where B
single verifications cost B of each.  The instance columns of every proof are committed through `Params.commit_batch` in chunks.

Soundness: the reference folds Horner-style (`acc.scale(r); acc.add_msm(m)`, batch.rs:79-89), i.e. weights r_{b+1} ... r_B that are
products of independent uniform scalars; here every weight is drawn independently, uniformly from the nonzero scalars.  If some
claim is not the identity, the weighted sum is a nonzero linear form in the r_b, which vanishes with probability at most 1/(q - 1)
over one independent r_b (Schwartz-Zippel, degree 1) -- no weaker than the reference's construction."""
from __future__ import annotations

import secrets
from dataclasses import dataclass

import numpy as np

from . import fields
from .arithmetic import ipa_s_combine
from .commitment import Blind, Params
from .verifier import MSM, VerificationError, VerifyingKey, _affine, _check_instances, _instance_lagrange, _verify_guard

INSTANCE_CHUNK = 8      # instance columns per commit_batch call: bounds the Lagrange vectors held on the device at once


@dataclass
class Claim:
    """One proof's verification equation before its s vector: `other` maps x -> [scalar, y] as MSM.other does; g0 is the G_0
    constant (-v) that `commitment_verify_proof` adds (a host scalar); neg_c and u give its s part, neg_c * compute_s(u, 1)."""
    other: dict
    w_scalar: int | None
    u_scalar: int | None
    g0: int
    neg_c: int
    u: list

    @classmethod
    def from_guard(cls, guard) -> "Claim":
        msm = guard.msm
        if msm.g_scalars is not None:
            raise ValueError("Claim.from_guard: the guard's MSM holds a device g vector (read it with MSM(params, defer_constant=True))")
        return cls({x: list(v) for x, v in msm.other.items()}, msm.w_scalar, msm.u_scalar, msm.g_constant or 0, guard.neg_c,
                   list(guard.u))


def draw_weights(count: int, field: int, rng=None) -> list[int]:
    """`count` independent uniformly random nonzero scalars.  Default source: the OS (`secrets`), as the reference uses OsRng;
    `rng(count)` -> (count, 4) Montgomery limbs follows create_proof's convention (a zero draw is drawn again)."""
    m = fields.MODULUS[field]
    if rng is None:
        return [secrets.randbelow(m - 1) + 1 for _ in range(count)]
    out = []
    while len(out) < count:
        out += [v % m for v in fields.from_limbs(np.ascontiguousarray(rng(count - len(out)), dtype=np.uint64).reshape(-1, 4), field, True)
                if v % m]
    return out


def combine_claims(params: Params, claims, weights) -> MSM:
    """sum_b weights[b] * claim_b as one MSM whose g part is a single (n, 4) device vector (see the module docstring)."""
    import torch
    msm = MSM(params)
    m, sf = msm.m, msm.sf
    claims, weights = list(claims), [w % m for w in weights]
    if len(claims) != len(weights):
        raise ValueError("combine_claims: one weight per claim")
    if not claims:
        return msm
    for c, r in zip(claims, weights):
        for x, (scalar, y) in c.other.items():
            msm.append_term(scalar * r % m, (x, y))
        if c.w_scalar is not None:
            msm.add_to_w_scalar(c.w_scalar * r)
        if c.u_scalar is not None:
            msm.add_to_u_scalar(c.u_scalar * r)
    for c in claims:
        if len(c.u) != params.k:
            raise ValueError("combine_claims: every claim needs k challenges")
    g = torch.empty((params.n, 4), dtype=torch.int64, device=fields.current_device())
    ipa_s_combine(params.k, np.stack([fields.to_limbs(c.u, sf, True) for c in claims]),
                  fields.to_limbs([r * c.neg_c % m for c, r in zip(claims, weights)], sf, True), sf, g)
    # index 0 of every s vector is the empty product 1, so g[0] = sum r_b neg_c_b; the G_0 constants join it there
    g[0] = torch.from_numpy(fields.scalar_limbs(sum(r * (c.neg_c + c.g0) for c, r in zip(claims, weights)) % m, sf, True).view(np.int64))
    msm.g_scalars = g
    return msm


def commit_instances(params: Params, vk: VerifyingKey, items):
    """The instance commitments of every item, [item][circuit instance][column] -> (x, y), by `Params.commit_batch` over
    g_lagrange in chunks of INSTANCE_CHUNK columns (blind = Blind::default(), plonk/verifier.rs:77-101)."""
    sf = vk.domain.field
    dev = fields.current_device()
    flat = [values for instances, _ in items for columns in instances for values in columns]
    points = []
    for lo in range(0, len(flat), INSTANCE_CHUNK):
        lags = [_instance_lagrange(params, values, sf, dev) for values in flat[lo:lo + INSTANCE_CHUNK]]
        jac = params.commit_batch(lags, [Blind(field=sf)] * len(lags), lagrange=True).cpu().numpy().view(np.uint64)
        points += [_affine(params, row) for row in jac]
        del lags
    out, pos = [], 0
    for instances, _ in items:
        per_item = []
        for columns in instances:
            per_item.append(points[pos:pos + len(columns)])
            pos += len(columns)
        out.append(per_item)
    return out


class BatchVerifier:
    """plonk/verifier/batch.rs:46-127: `add_proof(instances, proof)` any number of times, then `finalize(params, vk)` -> True iff
    every proof verifies (with high probability).  instances[i] = the instance columns of circuit instance i, as for
    verify_proof_many.  One verifying key per batch, as the reference."""

    def __init__(self):
        self.items = []

    def add_proof(self, instances, proof: bytes) -> None:
        self.items.append(([[list(col) for col in columns] for columns in instances], bytes(proof)))

    def claims(self, params: Params, vk: VerifyingKey):
        """Every item read up to its Claim; raises VerificationError on the first item that fails to parse or is malformed."""
        for instances, _ in self.items:
            _check_instances(params, vk, instances)
        commitments = commit_instances(params, vk, self.items)
        return [Claim.from_guard(_verify_guard(params, vk, instances, proof, MSM(params, defer_constant=True), instance_commitments=cms))
                for (instances, proof), cms in zip(self.items, commitments)]

    def finalize(self, params: Params, vk: VerifyingKey, rng=None) -> bool:
        """An empty batch is True (`params.empty_msm().eval()`); any parse or verification error of any item is False."""
        if not self.items:
            return True
        try:
            claims = self.claims(params, vk)
        except VerificationError:
            return False
        return combine_claims(params, claims, draw_weights(len(claims), vk.domain.field, rng)).eval()
