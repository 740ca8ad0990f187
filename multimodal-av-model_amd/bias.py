"""Contextual phrase biasing (hot words) for CTC prefix beam search (beam_search.prefix_beam_search(bias=...), csrc/context_bias.h,
csrc/ctc_beam.hip).

``ContextBias`` is a set P of distinct phrases over TOKEN IDS - 1..32 ids each, none of them the blank - over a vocabulary of
V <= 65533 ids.  The set has ONE weight, given to the search and not stored here: float32 nats per matched token, finite, may be negative.

The law (one wording for this file, csrc/context_bias.h and DESIGN §0.0f).  The state of a prefix is (k, tail), (0, ()) for the empty
prefix.  Per token c: tail <- the longest suffix of tail + (c) that is a prefix of some phrase of P (it may be empty); if tail is in P,
k <- k + |tail| and tail <- ().  Matches are therefore leftmost and non-overlapping and a completed phrase is banked.
m = k + |tail|: k is the banked credit, |tail| the refundable credit of a running partial match.  The search ranks a prefix by its score
plus weight * m and takes the refundable part back after the last frame (beam_search.prefix_beam_search).  m is a function of the prefix's
content alone, whatever the phrase set.  Two consequences, which are the law and not defects:
  - a phrase that is a proper prefix of another phrase always wins over it (``ab`` is banked before ``abc`` can complete);
  - a phrase that occurs strictly inside a longer partial match that later fails is not credited (with ``xabz`` and ``ab``, the text
    ``xabq`` holds ``ab`` but credits nothing: the running match of ``xabz`` owned those tokens).
``nested`` lists the phrases that are a contiguous part of another phrase, which is where either can happen.

Device tables (``to_device``): the trie of P, node 0 = the root.  ``nodes`` int32 [node_count][2] = (failure link, depth | terminal << 16);
the failure link is the deepest node that spells a proper suffix of the node's path.  Edges in the n-gram table's open-addressing form
(lm.py): 16-byte slots {u64 key, i32 child, i32 0}, power-of-two size, load <= 0.5, key 0 = empty, linear probing from
splitmix64(key) & (slots - 1), the longest probe run of a stored key recorded as the bound of every lookup; key = (node << 16) | (c + 1)."""
from __future__ import annotations

import os

import numpy as np

from .lm import MAX_VOCAB, splitmix64

MAX_PHRASE = 32
_SPACE = "▁"


class DeviceBias:
    """The tables of one ContextBias on one device (ContextBias.to_device)."""

    def __init__(self, nodes, edges, node_count, slots, probe_bound):
        self.nodes, self.edges, self.node_count, self.slots, self.probe_bound = nodes, edges, int(node_count), int(slots), int(probe_bound)


class ContextBias:
    def __init__(self, phrases, vocab_size, blank):
        """phrases: distinct tuples of ids, already checked (from_phrases is the public constructor)."""
        self.vocab_size, self.blank = int(vocab_size), int(blank)
        self.phrases = [tuple(p) for p in phrases]
        # the trie: children[node] = {token: child}; the path of node 0 is ()
        self.children, self.depth, self.terminal = [{}], [0], [False]
        for p in self.phrases:
            node = 0
            for c in p:
                nxt = self.children[node].get(c)
                if nxt is None:
                    nxt = len(self.children)
                    self.children[node][c] = nxt
                    self.children.append({}); self.depth.append(self.depth[node] + 1); self.terminal.append(False)
                node = nxt
            self.terminal[node] = True
        # failure links, breadth first: fail(child of n by c) = goto(fail(n), c)
        self.fail = [0] * len(self.children)
        queue = list(self.children[0].values())
        while queue:
            n = queue.pop(0)
            for c, ch in self.children[n].items():
                f = self.fail[n]
                while f and c not in self.children[f]:
                    f = self.fail[f]
                self.fail[ch] = self.children[f].get(c, 0)
                queue.append(ch)
        have = set(self.phrases)
        self.nested = sorted({p[i:j] for p in self.phrases for i in range(len(p)) for j in range(i + 1, len(p) + 1)
                              if j - i < len(p) and p[i:j] in have})
        self._devices = {}

    # ---- construction ----
    @classmethod
    def from_phrases(cls, phrases, tokenizer=None, vocab_size=None, blank=None):
        """phrases: strings (encoded with ``tokenizer.encode``: per character, a space - a leading one too - is the piece '▁', which is how
        a phrase is anchored at a word start) or sequences of ids (taken as given).  vocab_size and blank default to the tokenizer's.
        Duplicates are dropped.  ValueError, naming the phrase, for an empty phrase, one of more than 32 ids, one that holds the blank,
        an id outside [0, vocab_size) or a character the tokenizer does not know."""
        if vocab_size is None or blank is None:
            if tokenizer is None:
                raise ValueError("ContextBias.from_phrases: vocab_size and blank are needed without a tokenizer")
            vocab_size = tokenizer.vocab_size if vocab_size is None else vocab_size
            blank = tokenizer.blank_id if blank is None else blank
        V, blank = int(vocab_size), int(blank)
        if not 2 <= V <= MAX_VOCAB or not 0 <= blank < V:
            raise ValueError(f"ContextBias: need 2 <= vocab_size <= {MAX_VOCAB} and 0 <= blank < vocab_size, got {V}, {blank}")
        out, seen = [], set()
        for ph in phrases:
            if isinstance(ph, str):
                if tokenizer is None:
                    raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} is text and there is no tokenizer")
                ids = tuple(int(i) for i in tokenizer.encode(ph))
                known = tokenizer.token_to_id
                bad = [ch for ch in ph if (_SPACE if ch == " " else ch) not in known]
                if bad:
                    raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} holds {bad[0]!r}, which the tokenizer encodes as <unk>")
            else:
                ids = tuple(int(i) for i in ph)
            if not ids:
                raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} is empty")
            if len(ids) > MAX_PHRASE:
                raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} has {len(ids)} ids, more than {MAX_PHRASE}")
            if any(not 0 <= i < V for i in ids):
                raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} holds an id outside [0, {V})")
            if blank in ids:
                raise ValueError(f"ContextBias.from_phrases: phrase {ph!r} holds the blank {blank}")
            if ids not in seen:
                seen.add(ids)
                out.append(ids)
        return cls(out, V, blank)

    @classmethod
    def from_file(cls, path, tokenizer):
        """UTF-8 text, one phrase per line (the line ending is not part of it, a leading space is); blank lines and lines that start with
        ``#`` are skipped."""
        with open(os.fspath(path), encoding="utf-8") as f:
            lines = [ln.rstrip("\r\n") for ln in f]
        return cls.from_phrases([ln for ln in lines if ln.strip() and not ln.lstrip().startswith("#")], tokenizer)

    # ---- the law ----
    def step(self, node: int, k: int, c: int):
        """(node, k) of a prefix -> (node, k) of the prefix + (c): the transition of csrc/context_bias.h.  An id that no phrase can hold
        (the blank, or outside the vocabulary) matches nothing and ends a running match."""
        c = int(c)
        if not 0 <= c < self.vocab_size or c == self.blank:
            return 0, k
        while node and c not in self.children[node]:
            node = self.fail[node]
        node = self.children[node].get(c, 0)
        if self.terminal[node]:
            return 0, k + self.depth[node]
        return node, k

    def count(self, ids) -> np.ndarray:
        """int32 [len(ids)][2] = (k, |tail|) after each token of ``ids``: the host law."""
        out = np.zeros((len(ids), 2), np.int32)
        node = k = 0
        for i, c in enumerate(ids):
            node, k = self.step(node, k, c)
            out[i] = (k, self.depth[node])
        return out

    def banked(self, ids) -> int:
        """k of the whole sequence: what the search credits a finished hypothesis with."""
        c = self.count(ids)
        return int(c[-1, 0]) if len(c) else 0

    # ---- device tables ----
    def host_tables(self, slots=None):
        """(nodes int32 [node_count][2], edges int64 [slots][2] = the 16-byte slots, slots, probe bound)."""
        edges = {(n << 16) | (c + 1): ch for n, kids in enumerate(self.children) for c, ch in kids.items()}
        need = 2
        while need < 2 * len(edges):
            need *= 2
        slots = need if slots is None else int(slots)
        if slots < need or slots & (slots - 1):
            raise ValueError(f"ContextBias.to_device: slots {slots} must be a power of two >= {need} (load <= 0.5)")
        tab = np.zeros(slots, dtype=[("key", "<u8"), ("child", "<i4"), ("zero", "<i4")])
        keys = tab["key"]
        bound = 1
        for key, ch in edges.items():
            i, run = splitmix64(key) & (slots - 1), 1
            while keys[i] != 0:
                i, run = (i + 1) & (slots - 1), run + 1
            tab[i] = (key, ch, 0)
            bound = max(bound, run)
        nodes = np.stack([np.asarray(self.fail, np.int32),
                          np.asarray(self.depth, np.int32) | (np.asarray(self.terminal, np.int32) << 16)], axis=1)
        return np.ascontiguousarray(nodes), tab.view("<i8").reshape(slots, 2), slots, bound

    def to_device(self, device, slots=None) -> DeviceBias:
        import torch
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:                   # "cuda" and "cuda:0" are one device: one copy of the tables
            device = torch.device("cuda", torch.cuda.current_device())
        hit = self._devices.get((str(device), slots))
        if hit is None:
            nodes, tab, slots_, bound = self.host_tables(slots)
            hit = DeviceBias(torch.from_numpy(nodes).to(device), torch.from_numpy(tab).to(device), len(nodes), slots_, bound)
            self._devices[(str(device), slots)] = hit
        return hit

    def count_batch(self, ids, lens=None):
        """ids int32 [B][Lmax] on the GPU (lens [B], default Lmax, clamped to [0, Lmax]) -> int32 [B][Lmax][2] = (k, |tail|) after each
        token and 0 past the length: av_context_bias_count, one thread per sequence.  For scoring given text, n-best lists for instance."""
        import torch
        from . import _lib as L
        from . import ops
        if not ids.is_cuda or ids.dim() != 2:
            raise ValueError("ContextBias.count_batch: ids must be a [B, Lmax] tensor on the GPU")
        ids = ids.to(torch.int32).contiguous()
        B, Lmax = ids.shape
        ln = None if lens is None else torch.as_tensor(lens).to(device=ids.device, dtype=torch.long).contiguous()
        d = self.to_device(ids.device)
        out = torch.empty((B, Lmax, 2), dtype=torch.int32, device=ids.device)
        L.check(L.lib().av_context_bias_count(ops.ptr(ids), ops.ptr(ln), ops.ptr(out), B, Lmax, self.vocab_size, self.blank, ops.ptr(d.nodes),
                                              ops.ptr(d.edges), d.node_count, d.slots, d.probe_bound, ops.stream()), "av_context_bias_count")
        return out
