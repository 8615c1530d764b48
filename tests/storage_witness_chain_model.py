"""A host model of zkw_storage_tree_advance_witness_chain on top of tests/storage_witness_model.py: the sequential Table.advance per block,
then the restriction of each pre-state to the block's own keys. A helper, no test: tests/test_storage_witness_chain_model.py pins it against
the oracle's sequential tree, tests/test_gpu_storage_witness_chain.py uses it as a yardstick.

A block is its deduplicated storage queue as a list of (key, value, is_write) in queue order: a read counts for the block's key set and
writes nothing."""
from tests import storage_witness_model as model


def restrict(table, keys):
    """the table's state over `keys` only"""
    out = model.Table([], [], [], [], table.root, table.next_enumeration_index)
    out.entries = {k: table.entries[k] for k in keys}
    return out


def block_of(queries, derive_final_address):
    return [(derive_final_address(q), model.written_value(q), bool(q["rw_flag"])) for q in queries]


def chain(table, blocks):
    """([the table of block k's distinct keys in the state after blocks 0 .. k - 1], the table after the last block);
    KeyError((block, position)) for the first query, a read or a write, whose key is outside the table"""
    for b, block in enumerate(blocks):
        for pos, (k, _v, _w) in enumerate(block):
            if k not in table.entries:
                raise KeyError((b, pos))
    outs = []
    for block in blocks:
        outs.append(restrict(table, {k for k, _v, _w in block}))
        table = table.advance([(k, v) for k, v, w in block if w])
    return outs, table
