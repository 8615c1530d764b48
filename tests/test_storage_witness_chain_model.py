"""The host model of a chain of blocks (tests/storage_witness_chain_model.py) against the oracle's tree with sequential insert_leaf: a tree
of 300 leaves, a table of 120 keys and six blocks with the shapes the device schedule can go wrong at — block k + 1 writing the level-0
sibling of the key block k wrote, the same with keys that differ in bit 255 only, an empty block, a reads-only block, one key written in
every block (absent at first, three times in one block, once with the zero value), a read of a key an earlier block wrote. Every out[k] is
the oracle's answers for the block's distinct keys in the state BEFORE block k, the final table its answers for all keys after the last
block. No GPU: this pins the yardstick the GPU tests use."""
import numpy as np
import pytest

from tests import storage_witness_chain_model as chain_model
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


def test_chain_model_follows_the_oracle_tree(oracle):
    rng = np.random.default_rng(43)
    leaves = [rng.bytes(32) for _ in range(300)]
    tree = oracle.Tree()
    for k in leaves:
        tree.insert_leaf(k, rng.bytes(32))
    x, y, every = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    absent = [rng.bytes(32) for _ in range(45)] + [x, _flip(x, 0), y, _flip(y, 255), every]
    present = leaves[:70]
    keys = present + absent
    assert len(set(keys)) == 120
    table = _oracle_table(tree, keys)
    W, R = True, False
    w = lambda k: (k, rng.bytes(32), W)  # noqa: E731
    r = lambda k: (k, bytes(32), R)  # noqa: E731
    blocks = [
        [w(x), w(every), r(present[3]), w(present[4]), w(y)] + [w(k) for k in absent[:10]],
        [w(_flip(x, 0)), w(_flip(y, 255)), w(every), r(absent[20]), w(every), w(every), w(present[4])],
        [],
        [r(x), r(present[4]), (every, bytes(32), W), w(absent[20]), r(absent[21])] + [w(k) for k in present[10:40]],
        [r(every), r(absent[20]), r(present[5])],
        [w(every), w(absent[21]), w(_flip(x, 0))],
    ]
    outs, final = chain_model.chain(table, blocks)
    assert len(outs) == len(blocks)
    index_of_every = set()
    for block, out in zip(blocks, outs):
        block_keys = sorted({k for k, _v, _w in block})
        assert sorted(out.entries) == block_keys
        _same(out, _oracle_table(tree, block_keys))
        if every in out.entries:
            index_of_every.add(out.entries[every][0])
        for k, v, is_write in block:
            if is_write:
                tree.insert_leaf(k, v)
    _same(final, _oracle_table(tree, keys))
    assert index_of_every == {0, 301 + 1}  # absent before block 0, then the index of block 0's second new key, kept through the zero value
    assert outs[2].entries == {} and outs[2].root == outs[3].root != outs[1].root  # the empty block carries the state
    assert outs[5].root == outs[4].root and outs[5].next_enumeration_index == outs[4].next_enumeration_index  # and so does the reads-only one
    assert outs[3].entries[x][0] == 301 and outs[4].entries[every][1] == bytes(32)
    with pytest.raises(KeyError) as ei:
        chain_model.chain(table, [[r(keys[0])], [w(keys[1]), r(rng.bytes(32)), w(rng.bytes(32))], [r(rng.bytes(32))]])
    assert ei.value.args == ((1, 1),)
