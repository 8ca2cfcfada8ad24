"""Pedersen vector commitments over Grumpkin (bn_amd.grumpkin): C = sum of [v_i] G_i (+ [blind] H), one bn_amd.grumpkin_msm_batch per call - a
pairing-free commitment whose points have coordinates in Fr, so a circuit over Fr opens it natively.

The generators are derived by try-and-increment:

    x = int(SHA-256(label | be32(index) | be32(ctr)), big endian) mod r        for ctr = 0, 1, 2, ..
    the first ctr for which x^3 - 17 is a square mod r wins;  y = the root that is not above (r - 1) / 2

THIS DERIVATION IS THIS PROJECT'S OWN.  It is NOT Barretenberg's (Aztec's generators come from its own hash-to-curve and domain separators) and
not any other library's: commitments made here agree with nothing but this module.  Nobody knows a discrete logarithm between two of these
points unless SHA-256 is broken, which is all the binding property needs.  The values and blinds are integers mod q (the group order)."""
import hashlib

from . import grumpkin as GK
from .babyjub import sqrt_host

BLIND_LABEL = b"bn_amd.pedersen.blind"


def generators(n, label):
    """[n grumpkin.Point] for the label (str or bytes): generator i depends on (label, i) only, so a longer list extends a shorter one"""
    label = label if isinstance(label, bytes) else label.encode()
    out = []
    for i in range(n):
        ctr = 0
        while True:
            x = int.from_bytes(hashlib.sha256(label + i.to_bytes(4, "big") + ctr.to_bytes(4, "big")).digest(), "big") % GK.R
            y = sqrt_host(x * x * x + GK.B)
            if y is not None:
                break
            ctr += 1
        out.append(GK.Point(x, y))
    return out


def blind_generator():
    """H: the point the blind multiplies when the caller names none"""
    return generators(1, BLIND_LABEL)[0]


def _terms(gens, values, blind, h):
    values = [int(v) % GK.Q for v in values]
    if len(values) > len(gens):
        raise ValueError(f"{len(values)} values, {len(gens)} generators")
    pts, ks = list(gens[:len(values)]), values
    if blind is not None:
        pts, ks = pts + [h], ks + [int(blind) % GK.Q]
    return pts, ks


def commit(gens, values, blind=None, h=None, engine=None):
    """sum of [values[i]] gens[i], plus [blind] h when a blind is given (h: blind_generator() unless named) -> grumpkin.Point: ONE
    grumpkin_msm_batch of one segment.  Fewer values than generators use the first ones"""
    pts, ks = _terms(gens, values, blind, (h or blind_generator()) if blind is not None else None)
    return GK.grumpkin_msm_batch(pts, ks, [0, len(pts)], engine=engine)[0]


def commit_batch(gens, vectors, blinds=None, h=None, engine=None):
    """[commit(gens, v, blind)] for many vectors against the same generators: ONE grumpkin_msm_batch of len(vectors) segments"""
    vectors = [list(v) for v in vectors]
    if blinds is not None and len(blinds) != len(vectors):
        raise ValueError(f"{len(vectors)} vectors, {len(blinds)} blinds")
    hh = (h or blind_generator()) if blinds is not None else None
    pts, ks, offs = [], [], [0]
    for j, v in enumerate(vectors):
        p, k = _terms(gens, v, None if blinds is None else blinds[j], hh)
        pts += p; ks += k; offs.append(len(pts))
    return GK.grumpkin_msm_batch(pts, ks, offs, engine=engine)


def commit_host(gens, values, blind=None, h=None):
    """the same sum in host integers (the model the tests compare with)"""
    pts, ks = _terms(gens, values, blind, (h or blind_generator()) if blind is not None else None)
    acc = GK.IDENTITY
    for p, k in zip(pts, ks):
        acc = GK.add_host(acc, GK.mul_host((p.x, p.y), k))
    return GK.Point(*acc)
