"""A host model of zkw_storage_tree_advance_witness in plain Python, on dictionaries, with hashlib's Blake2s: the table of a key set (index,
value, Merkle path per key) in the state after a batch of writes, computed from the table before it and nothing else. A helper, no test:
tests/test_storage_witness_advance_model.py pins it against the oracle's sequential tree, tests/test_gpu_storage_witness_advance.py uses it
as a yardstick beside the full device tree.

The rule. A key is the 256-bit number of its 32 little-endian bytes; bit L decides the side at level L (0 = the leaves). The written keys
W fold upwards level by level: node[0][k] = the new leaf hash, node[L + 1][k >> (L + 1)] = H(left, right) of node[L][k >> L] and its
sibling, which is node[L][(k >> L) ^ 1] when a written key lies under the sibling, else the OLD path[L] of k (a subtree without a written
key keeps its hash). Every entry's new path[L] is node[L][(key >> L) ^ 1] where that exists, else its old path[L]."""
import hashlib

import numpy as np


def _h(x):
    return hashlib.blake2s(x, digest_size=32).digest()


def leaf_hash(index, value):
    return _h(int(index).to_bytes(8, "big") + value)


def fold(key, index, value, path):
    """the root a proof leads to"""
    bits, cur = int.from_bytes(key, "little"), leaf_hash(index, value)
    for lv in range(256):
        sib = bytes(path[lv])
        cur = _h(sib + cur) if (bits >> lv) & 1 else _h(cur + sib)
    return cur


def written_value(q):
    """a log query's written_value (U256 limbs) as the tree's 32 bytes"""
    return b"".join(int(x).to_bytes(4, "big") for x in q["written_value"][::-1])


class Table:
    """entries: key -> (index, value, [256 siblings]) of one state, with its root and next enumeration index"""

    def __init__(self, keys, indexes, values, paths, root, next_enumeration_index):
        self.entries = {bytes(k): (int(i), bytes(v), [bytes(s) for s in p]) for k, i, v, p in zip(keys, indexes, values, paths)}
        self.root, self.next_enumeration_index = bytes(root), int(next_enumeration_index)

    @property
    def num_leaves(self):
        return sum(1 for i, _v, _p in self.entries.values() if i)

    def advance(self, pairs):
        """the table after insert(key, value) of the pairs one after another; KeyError(position) for a key outside the table"""
        for pos, (k, _v) in enumerate(pairs):
            if k not in self.entries:
                raise KeyError(pos)
        new_index, value, nxt = {}, {}, self.next_enumeration_index
        for k, v in pairs:
            if k not in new_index:  # first occurrence: an absent key becomes present, in array order
                old = self.entries[k][0]
                if old == 0:
                    old, nxt = nxt, nxt + 1
                new_index[k] = old
            value[k] = v  # the last value stays
        nodes = {int.from_bytes(k, "little"): (leaf_hash(new_index[k], value[k]), self.entries[k][2]) for k in new_index}
        levels = [{n: h for n, (h, _p) in nodes.items()}]
        for lv in range(256):
            up = {}
            for n, (h, path) in nodes.items():
                if n >> 1 in up:
                    continue  # its written sibling has made the parent
                sib = nodes[n ^ 1][0] if n ^ 1 in nodes else path[lv]
                up[n >> 1] = (_h(sib + h) if n & 1 else _h(h + sib), path)
            nodes = up
            levels.append({n: h for n, (h, _p) in nodes.items()})
        out = Table([], [], [], [], levels[256][0] if new_index else self.root, nxt)
        for k, (i, v, path) in self.entries.items():
            n = int.from_bytes(k, "little")
            out.entries[k] = (new_index.get(k, i), value.get(k, v), [levels[lv].get((n >> lv) ^ 1, path[lv]) for lv in range(256)])
        return out

    def advance_by_queries(self, queries, derive_final_address):
        return self.advance([(derive_final_address(q), written_value(q)) for q in queries if q["rw_flag"]])

    def answers(self, keys):
        """(leaf_indexes [n] uint64, values [n, 32], merkle_paths [n, 256, 32]) as get_leaves gives them"""
        idx = np.array([self.entries[k][0] for k in keys], np.uint64)
        val = np.frombuffer(b"".join(self.entries[k][1] for k in keys), np.uint8).reshape(-1, 32)
        paths = np.frombuffer(b"".join(b"".join(self.entries[k][2]) for k in keys), np.uint8).reshape(-1, 256, 32)
        return idx, val, paths
