"""The host model of the advance of a witness tree (tests/storage_witness_model.py) against the oracle's tree with sequential insert_leaf:
a tree of 370 leaves, a table of 216 keys with the edge shapes — the all-zero and all-ones keys, pairs that differ in bit 0 only and in bit
255 only, 64 keys under one node of height 6, absent neighbours of present keys — and four consecutive batches of 0, 1, 47 and 150 writes
with repeats, new keys and a zero value to an absent key. Indices, values, all 256 levels of every path, roots and next enumeration indices
are the oracle's, exactly. No GPU: this pins the yardstick the GPU tests use."""
import numpy as np
import pytest

from tests import storage_witness_model as model


def _flip(key, bit):
    k = bytearray(key)
    k[bit // 8] ^= 1 << (bit % 8)
    return bytes(k)


def _oracle_table(tree, keys):
    answers = [tree.get_leaf(k) for k in keys]
    return model.Table(keys, [a[0] for a in answers], [a[1] for a in answers], [a[2] for a in answers], tree.root, tree.next_enumeration_index)


def _same(a, b):
    assert a.root == b.root and a.next_enumeration_index == b.next_enumeration_index and a.num_leaves == b.num_leaves
    assert a.entries.keys() == b.entries.keys()
    for k in a.entries:
        assert a.entries[k] == b.entries[k], k.hex()


def test_model_follows_the_oracle_tree(oracle):
    rng = np.random.default_rng(41)
    a, b, c = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    run = [bytes([i]) + c[1:] for i in range(64)]  # 64 keys under one node of height 6
    edge = [bytes(32), b"\xff" * 32, a, _flip(a, 0), b, _flip(b, 255)] + run
    leaves = [rng.bytes(32) for _ in range(370 - len(edge))] + edge
    tree = oracle.Tree()
    for k in leaves:
        tree.insert_leaf(k, rng.bytes(32))
    neighbours = [_flip(run[0], 6), _flip(run[63], 255), _flip(a, 1), _flip(bytes(32), 0), _flip(b"\xff" * 32, 255), _flip(c, 255)]
    neighbours.append(_flip(neighbours[-1], 0))  # two absent keys that differ in bit 0 only
    present = [leaves[i] for i in rng.choice(370 - len(edge), size=70, replace=False)] + edge
    absent = [rng.bytes(32) for _ in range(216 - len(present) - len(neighbours))] + neighbours
    keys = present + absent
    assert len(keys) == len(set(keys)) == 216 and not set(absent) & set(leaves)
    table = _oracle_table(tree, keys)
    assert table.num_leaves == len(present)
    for k in (keys[0], keys[-1]):
        assert model.fold(k, *table.entries[k]) == tree.root

    def batch(n):
        ks = [keys[i] for i in rng.integers(0, len(keys), size=n)]  # repeats, present and absent
        return [(k, rng.bytes(32)) for k in ks]

    batches = [[], batch(1), batch(47), batch(150)]
    batches[2][5:5] = [(neighbours[-1], bytes(32)), (neighbours[-2], rng.bytes(32))]  # a zero value to an absent key, and its sibling
    batches[3] += [(k, rng.bytes(32)) for k in run] + [(batches[3][0][0], rng.bytes(32))] * 2
    for n_batch, pairs in enumerate(batches):
        before = tree.next_enumeration_index
        for k, v in pairs:
            tree.insert_leaf(k, v)
        table = table.advance(pairs)
        _same(table, _oracle_table(tree, keys))
        new = len({k for k, _v in pairs} - set(leaves))
        leaves += list({k for k, _v in pairs})
        assert table.next_enumeration_index == before + new
        if n_batch == 2:  # a zero value took an index
            assert table.entries[neighbours[-1]][0] != 0 and table.entries[neighbours[-1]][1] == bytes(32)
    with pytest.raises(KeyError) as ei:
        table.advance([(keys[0], bytes(32)), (rng.bytes(32), bytes(32))])
    assert ei.value.args == (1,)
