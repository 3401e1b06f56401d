"""Ending rules of text generation beyond the one ``eos_token_id`` ("ending rules"): a set of stop tokens, up
to 16 stop sequences of 1 .. 8 token ids, and ``min_new_tokens``.  ``StopRules`` validates on the host, builds the arrays the
sampler reads (``tcavt_stop_rules``, include/tcavt.h) and -- ``first_end`` -- states the rules on a plain token list, which is what the
tests hold the kernels to.

HF correspondences: the stop set is ``generate(eos_token_id=[eos, *stop_token_ids])`` (``EosTokenCriteria``: the token is kept);
``min_new_tokens`` is ``MinNewTokensLengthLogitsProcessor`` over that same list; a stop sequence is a stopping criterion on the
generated ids only (it never matches across the end of the prompt) and, like every stopping criterion, does not look at
``min_new_tokens``."""
import ctypes

import torch

from . import capi

MAX_SEQS = 16
MAX_SEQ_LEN = 8
RUNNING, EOS, STOP_TOKEN, STOP_SEQUENCE, BUDGET = 0, 1, 2, 3, 4  # finish_reason; when several apply in one step the smallest wins


class StopRules:
    def __init__(self, vocab, stop_token_ids=None, stop_sequences=None, min_new_tokens=0):
        self.vocab = int(vocab)
        if self.vocab < 1:
            raise ValueError(f"StopRules: vocab must be >= 1, got {vocab}")
        ids = [int(t) for t in (stop_token_ids if stop_token_ids is not None else ())]
        for t in ids:
            if not 0 <= t < self.vocab:
                raise ValueError(f"StopRules: stop token id {t} outside [0, vocab = {self.vocab})")
        seqs = [[int(t) for t in s] for s in (stop_sequences if stop_sequences is not None else ())]
        if len(seqs) > MAX_SEQS:
            raise ValueError(f"StopRules: {len(seqs)} stop sequences, at most {MAX_SEQS}")
        for s in seqs:
            if not 1 <= len(s) <= MAX_SEQ_LEN:
                raise ValueError(f"StopRules: a stop sequence has 1 .. {MAX_SEQ_LEN} ids, got {len(s)}")
            for t in s:
                if not 0 <= t < self.vocab:
                    raise ValueError(f"StopRules: stop sequence id {t} outside [0, vocab = {self.vocab})")
        # one minimum, or one per request: then the struct's own stays 0 and the sampler reads the request table's (the generate
        # entries check the elements, with their index, when they build it)
        if isinstance(min_new_tokens, torch.Tensor) and min_new_tokens.dim() >= 1:
            min_new_tokens = min_new_tokens.tolist()
        self.min_new_per_request = tuple(min_new_tokens) if isinstance(min_new_tokens, (list, tuple)) else None
        self.min_new_tokens = 0 if self.min_new_per_request is not None else int(min_new_tokens)
        if self.min_new_tokens < 0:
            raise ValueError(f"StopRules: min_new_tokens must be >= 0, got {min_new_tokens}")
        self.stop_token_ids = tuple(sorted(set(ids)))
        self.stop_sequences = tuple(tuple(s) for s in seqs)
        # bitmap: bit (id & 31) of word (id >> 5); int32 storage of the uint32 words
        words = [0] * ((self.vocab + 31) // 32)
        for t in self.stop_token_ids:
            words[t >> 5] |= 1 << (t & 31)
        self.bitmap = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32)
        self.seqs = torch.zeros(max(len(seqs), 1), MAX_SEQ_LEN, dtype=torch.int64)
        self.seq_len = torch.zeros(max(len(seqs), 1), dtype=torch.int32)
        for q, s in enumerate(seqs):
            self.seqs[q, :len(s)] = torch.tensor(s, dtype=torch.int64)
            self.seq_len[q] = len(s)

    @property
    def empty(self):
        """No rule at all: the sampler runs exactly as without rules."""
        return not self.stop_token_ids and not self.stop_sequences and self.min_new_tokens == 0 and not any(self.min_new_per_request or ())

    def min_new(self, request=None):
        """The minimum of request ``request`` (the one minimum when it is not given per request)."""
        return self.min_new_tokens if self.min_new_per_request is None or request is None else int(self.min_new_per_request[request])

    def check_bannable(self, min_new_tokens, eos_token_id):
        """A positive minimum needs something to ban: the request's own eos_token_id or the stop set."""
        if min_new_tokens > 0 and (eos_token_id is None or eos_token_id < 0) and not self.stop_token_ids:
            raise ValueError("StopRules: min_new_tokens needs eos_token_id or stop_token_ids (nothing to ban)")

    def to(self, device):
        """The arrays on ``device`` (one upload per call of a generate entry): a DeviceStopRules."""
        return DeviceStopRules(self, device)

    def first_end(self, tokens, eos_token_id, budget=None, request=None):
        """Where a request that generates ``tokens`` (its own tokens only, no prompt) ends: -> (n_generated, reason).  Token i ends
        it -- in this order of precedence -- as EOS (1), as a stop token (2), when the last n tokens up to and including it equal a
        stop sequence of length n <= i + 1 (3), or when i + 1 == budget (4).  None of the rules fires: (len(tokens), 0).  The ban
        before ``min_new_tokens`` acts on the scores, not here: a banned token cannot appear in ``tokens`` to begin with.  ``request``
        (with per-request minima, and eos_token_id then the request's own): the request's minimum is taken -- an ending token
        before it is a token the sampler cannot have emitted, which is an error of the caller's token list."""
        toks = [int(t) for t in tokens]
        stop = set(self.stop_token_ids)
        floor = self.min_new(request) if request is not None else 0
        for i, t in enumerate(toks):
            is_eos = eos_token_id is not None and eos_token_id >= 0 and t == int(eos_token_id)
            if i < floor and (is_eos or t in stop):
                raise ValueError(f"StopRules.first_end: token {i} = {t} of request {request} is banned before its minimum {floor}")
            if is_eos:
                return i + 1, EOS
            if t in stop:
                return i + 1, STOP_TOKEN
            for s in self.stop_sequences:
                if i + 1 >= len(s) and tuple(toks[i + 1 - len(s):i + 1]) == s:
                    return i + 1, STOP_SEQUENCE
            if budget is not None and i + 1 == int(budget):
                return i + 1, BUDGET
        return len(toks), RUNNING


class DeviceStopRules:
    """The device arrays of a StopRules plus the two per-request records, and the ``tcavt_stop_rules`` struct over them."""

    def __init__(self, rules, device):
        self.rules = rules
        self.bitmap = rules.bitmap.to(device) if rules.stop_token_ids else None
        n = len(rules.stop_sequences)
        self.seqs = rules.seqs.to(device) if n else None
        self.seq_len = rules.seq_len.to(device) if n else None
        self.finish_reason = self.n_generated = None
        self._struct = None

    def records(self, n_requests, device):
        """finish_reason / n_generated int32 [n_requests], zeroed; the sampler writes a request's pair when the request ends."""
        self.finish_reason = torch.zeros(n_requests, dtype=torch.int32, device=device)
        self.n_generated = torch.zeros(n_requests, dtype=torch.int32, device=device)
        self._struct = None
        return self

    def struct(self):
        if self._struct is None:
            s = capi.StopRules()
            capi.bind(s, stop_bitmap=self.bitmap, stop_seqs=self.seqs, stop_seq_len=self.seq_len, finish_reason=self.finish_reason,
                      n_generated=self.n_generated)
            s.n_seqs, s.min_new_tokens = len(self.rules.stop_sequences), self.rules.min_new_tokens
            self._struct = s
        return self._struct

    def pointer(self):
        return ctypes.pointer(self.struct())
