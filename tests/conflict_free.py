"""Conflict-free BPR triplet lists: inputs on which a parallel Hogwild epoch has ONE right answer.

The triplets come in blocks.  Block ``b`` owns users ``[b*nu, (b+1)*nu)`` and items ``[b*ni, (b+1)*ni)`` and nothing else touches them.
When the launched order puts every block inside one chunk, no two chunks share a row of P or Q: whatever the grid, the visiting order of
the chunks and the update policy (lossy load + store ones included), the result is the sequential recurrence over the stored order -- to
fp32 rounding against the fp64 oracle, and bit for bit against the same kernel run by one group.  Inside a block the rows are few, so the
same user, the same negative, a negative that is an earlier or a later positive and long runs of one positive all occur many times: the
register forwarding and flush paths of the kernels are exercised in every chunk, not only where a data set happens to repeat a row.

``chunks_are_row_disjoint`` is the precondition, checked by every test on the order it actually launches (read back from the device)."""
import numpy as np


def conflict_free_triplets(rng, n_blocks, block, users_per_block, items_per_block, tail=0):
    """(u, i, j), int32, block after block: ``block`` triplets each (the last one ``tail`` of them when ``tail`` > 0); positives from the
    lower half of the block's items, negatives from all of them with j != i (the samplers never draw a positive of the same triplet)"""
    nu, ni = int(users_per_block), int(items_per_block)
    assert n_blocks >= 1 and block >= 1 and nu >= 1 and ni >= 2 and 0 <= tail <= block
    n = (n_blocks - 1) * block + (tail if tail > 0 else block)
    b = (np.arange(n, dtype=np.int64) // block)
    u = b * nu + rng.integers(0, nu, n)
    i = b * ni + rng.integers(0, ni // 2, n)
    j = b * ni + rng.integers(0, ni, n)
    j = np.where(j == i, b * ni + ni - 1, j)          # ni - 1 lies in the upper half: never a positive
    return u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)


def _row_in_two_chunks(rows, chunk_of):
    o = np.lexsort((chunk_of, rows))
    r, c = rows[o], chunk_of[o]
    return bool(((r[1:] == r[:-1]) & (c[1:] != c[:-1])).any())


def chunks_are_row_disjoint(u, i, j, chunk):
    """the STORED order (u, i, j) cut into chunks of ``chunk``: True iff no user row and no item row (positives and negatives together)
    appears in two chunks"""
    u, i, j = (np.asarray(x).astype(np.int64) for x in (u, i, j))
    assert u.shape == i.shape == j.shape and u.ndim == 1 and chunk >= 1
    c = np.arange(u.size, dtype=np.int64) // int(chunk)
    return not _row_in_two_chunks(u, c) and not _row_in_two_chunks(np.concatenate([i, j]), np.concatenate([c, c]))


def chunks_in_order(n, chunk, chunk_order):
    """positions 0..n-1 with the chunks of ``chunk`` taken in ``chunk_order``, front to back inside each"""
    return np.concatenate([np.arange(c * chunk, min(n, (c + 1) * chunk), dtype=np.int64) for c in chunk_order])
