# Copyright 2026 mlrun_amd authors
#
# Licensed under the Apache License, Version 2.0 (the "License");
# you may not use this file except in compliance with the License.
"""Host index of the prefix cache: which pool block holds the KV rows
of which 32-token block of which prompt prefix.  Pure Python, no
tensors; the engine owns the pool and moves the rows
(``ops.kv_block_copy``)."""

from collections import OrderedDict

from ..ops import KV_BLOCK_TOKENS


class PrefixIndex:
    """(adapter id, chain of 32-token blocks) -> pool block id.

    A block's key is ``(parent pool id or -1, adapter id, its 32
    tokens)``, so a chain of keys spells the whole prefix: a hit means
    every token before the block's end, and the adapter id, are equal.
    Nothing is matched by hash alone.

    Eviction is least-recently-used over LEAF blocks only.  A block with
    children is never recycled, so no key can name a recycled id as its
    parent, and a chain in the index is always whole from its root.
    Blocks touched since ``begin()`` are pinned: one admission call
    gathers from and scatters into the pool after it has planned both,
    so none of its blocks may change owner in between."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise ValueError(f"prefix cache capacity {capacity} < 1")
        self.capacity = int(capacity)
        self.lookups = 0
        self.prompt_tokens = 0
        self.hit_tokens = 0
        self.inserted = 0
        self.evicted = 0
        self.clear()

    def clear(self):
        """Forget every block (the counters keep running)."""
        self._by_key = {}                 # key -> pool id
        self._blocks = OrderedDict()      # pool id -> [key, children], LRU
        self._free = list(range(self.capacity - 1, -1, -1))
        self._pinned = set()

    @property
    def blocks_in_use(self) -> int:
        return len(self._blocks)

    def begin(self):
        """Start an admission call: unpin the blocks of the last one."""
        self._pinned.clear()

    def _touch(self, block: int):
        self._blocks.move_to_end(block)
        self._pinned.add(block)

    @staticmethod
    def _key(parent: int, adapter: int, tokens, index: int):
        lo = index * KV_BLOCK_TOKENS
        return (parent, adapter, tuple(tokens[lo:lo + KV_BLOCK_TOKENS]))

    def lookup(self, tokens, adapter: int = -1) -> list:
        """Pool ids of the longest cached chain that starts ``tokens``
        under ``adapter``, at most (len(tokens) - 1) // 32 blocks so
        that one token at least is left to prefill.  Every returned
        block is touched."""
        adapter = int(adapter)
        chain, parent = [], -1
        for index in range((len(tokens) - 1) // KV_BLOCK_TOKENS):
            block = self._by_key.get(self._key(parent, adapter, tokens,
                                               index))
            if block is None:
                break
            self._touch(block)
            chain.append(block)
            parent = block
        self.lookups += 1
        self.prompt_tokens += len(tokens)
        self.hit_tokens += len(chain) * KV_BLOCK_TOKENS
        return chain

    def _evict(self):
        """Free the least recently used unpinned leaf; None if every
        block has children or is pinned."""
        for block, (key, children) in self._blocks.items():
            if children == 0 and block not in self._pinned:
                del self._blocks[block]
                del self._by_key[key]
                if key[0] >= 0:
                    self._blocks[key[0]][1] -= 1
                self.evicted += 1
                return block
        return None

    def insert(self, tokens, adapter: int = -1) -> list:
        """Enter the full 32-token blocks of ``tokens`` that are not yet
        cached; returns [(block index in the prompt, pool id)] for the
        new ones, in chain order: the caller copies those rows into the
        pool.  A full pool evicts LRU leaves; when none can go the chain
        stops there (a child is never entered without its parent)."""
        adapter = int(adapter)
        new, parent = [], -1
        for index in range(len(tokens) // KV_BLOCK_TOKENS):
            key = self._key(parent, adapter, tokens, index)
            block = self._by_key.get(key)
            if block is None:
                # the parent is a leaf now, but it was touched above
                # and so is pinned: evicting cannot take it
                block = self._free.pop() if self._free else self._evict()
                if block is None:
                    break
                self._by_key[key] = block
                self._blocks[block] = [key, 0]
                if parent >= 0:
                    self._blocks[parent][1] += 1
                self.inserted += 1
                new.append((index, block))
            self._touch(block)
            parent = block
        return new

    def stats(self) -> dict:
        return {"lookups": self.lookups,
                "prompt_tokens": self.prompt_tokens,
                "hit_tokens": self.hit_tokens,
                "inserted": self.inserted,
                "evicted": self.evicted,
                "blocks_in_use": self.blocks_in_use,
                "capacity": self.capacity}
