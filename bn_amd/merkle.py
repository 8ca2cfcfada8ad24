"""Binary Merkle trees of Poseidon over Fr on the GPU (Semaphore / Tornado style membership trees): a node is hash(left, right), the
circomlib / iden3 hash of arity 2 (bn_amd.poseidon).

Tree(leaves) builds every node with ONE bn_amd.fr_merkle_tree call (one launch per level); open(i) reads a path out of the nodes, which stay
on the host as integers; verify walks one path in host integers (bn_amd.poseidon.hash_host: no device); verify_batch checks m openings of one
depth with ONE fr_poseidon_batch of m hashes per level - left and right are chosen by the index bit on the host.  Tree.from_records hashes
variable-length records into the leaves with ONE bn_amd.fr_poseidon_chain_batch call first.

Not built: trees of arity 4, a several-lanes-per-hash kernel for the top levels (a level of one node is one lane's chain of about 830 dependent
products), sparse trees, updates in place."""
import numpy as np

from .api import Fr, _scalar_array, default_engine
from . import poseidon


class Tree:
    """the tree over n = 2^depth leaves (a sequence of Fr or an (n, 4) uint64 array): .leaves and .nodes are lists of Fr, the nodes level by
    level with the root last, .depth = log2 n"""

    def __init__(self, leaves, engine=None):
        from .engine import _merkle_args
        x, self.depth = _merkle_args(_scalar_array(leaves))
        self.leaves = [Fr.from_limbs(r) for r in x]
        self.nodes = [Fr.from_limbs(r) for r in (engine or default_engine()).fr_merkle_tree(x)]

    @classmethod
    def from_records(cls, rows, rate=16, engine=None):
        """the tree whose leaf i is the digest of the variable-length record rows[i] (bn_amd.poseidon.hash_chain_host: this package's own
        framing): ONE fr_poseidon_chain_batch call for the leaves, then the tree as above.  rows: a power of two of sequences of Fr, of any
        lengths"""
        from .api import fr_poseidon_chain_batch
        e = engine or default_engine()
        return cls(fr_poseidon_chain_batch(rows, rate=rate, engine=e), engine=e)

    @property
    def root(self):
        return self.nodes[-1] if self.nodes else self.leaves[0]

    def open(self, i):
        """the path of leaf i: its `depth` siblings, from the leaf level up"""
        n = len(self.leaves)
        if not 0 <= i < n:
            raise IndexError(f"leaf {i} of {n}")
        path, level, off = [], self.leaves, 0
        while n > 1:
            path.append(level[i ^ 1])
            level = self.nodes[off:off + n // 2]
            off += n // 2; n //= 2; i >>= 1
        return path


def verify(root, leaf, i, path):
    """leaf is leaf number i of the tree with this root, by its path - in host integers"""
    if not 0 <= i < 1 << len(path):
        return False
    cur = leaf.v
    for sib in path:
        cur = poseidon.hash_host([sib.v, cur] if i & 1 else [cur, sib.v])
        i >>= 1
    return cur == root.v


def verify_batch(root, leaves, indices, paths, engine=None):
    """[verify(root, leaf, i, path) for ..] -> list of bool, for m openings of ONE depth: per level one fr_poseidon_batch of m hashes.  An index
    outside the tree is False.  ValueError when the paths differ in length or the operands in number."""
    leaves, indices, paths = list(leaves), [int(i) for i in indices], [list(p) for p in paths]
    if not len(leaves) == len(indices) == len(paths):
        raise ValueError(f"{len(leaves)} leaves, {len(indices)} indices and {len(paths)} paths")
    if not leaves:
        return []
    depth = len(paths[0])
    if any(len(p) != depth for p in paths):
        raise ValueError(f"the paths differ in length: {sorted({len(p) for p in paths})}")
    e = engine or default_engine()
    cur = _scalar_array(leaves)
    idx = np.array([i if 0 <= i < 1 << depth else 0 for i in indices], np.int64)
    for level in range(depth):
        sib = _scalar_array([p[level] for p in paths])
        right = ((idx >> level) & 1).astype(bool)[:, None]
        cur = e.fr_poseidon_batch(np.stack([np.where(right, sib, cur), np.where(right, cur, sib)], axis=1))
    want = root.limbs
    return [bool((c == want).all()) and 0 <= i < 1 << depth for c, i in zip(cur, indices)]
