"""Token-automaton constraints of text generation ("constrained decoding"): the sampler may only emit
tokens that keep a row inside a form the caller can parse.  ``TokenConstraint`` is a deterministic automaton over token ids,
stored by token class -- ``token_class`` int32 [V] and ``trans`` int32 [n_states, n_classes], -1 = not allowed -- validated on the
host; the builders make the common ones, and ``walk`` / ``allowed`` state the rule on a plain token list, which is what the
tests hold the kernels (tcavt_constraint_build / _mask / _advance, include/tcavt.h) to.

HF correspondences: ``from_sequences`` and every other automaton are ``generate(prefix_allowed_tokens_fn=...)`` with the function
held on the device, ``from_allowed_tokens`` is an allowed vocabulary, ``from_suppressed_tokens`` is ``suppress_tokens``.  No
tokenizer is involved: everything is in token ids, as in ``stop_sequences``."""
import numbers

import torch

MAX_STATES = 4096
MAX_CLASSES = 4096


class TokenConstraint:
    def __init__(self, token_class, trans, start=0):
        token_class, trans = torch.as_tensor(token_class), torch.as_tensor(trans)
        if token_class.dim() != 1 or token_class.numel() < 1:
            raise ValueError(f"TokenConstraint: token_class must be a non-empty 1-D array [V], got shape {tuple(token_class.shape)}")
        if trans.dim() != 2 or trans.shape[0] < 1 or trans.shape[1] < 1:
            raise ValueError(f"TokenConstraint: trans must be a 2-D array [n_states, n_classes], got shape {tuple(trans.shape)}")
        for t, nm in ((token_class, "token_class"), (trans, "trans")):
            if t.dtype != torch.int32:
                raise ValueError(f"TokenConstraint: {nm} must be int32, got {t.dtype}")
        self.vocab = token_class.numel()
        self.n_states, self.n_classes = (int(d) for d in trans.shape)
        if self.n_states > MAX_STATES:
            raise ValueError(f"TokenConstraint: {self.n_states} states, at most {MAX_STATES}")
        if self.n_classes > MAX_CLASSES:
            raise ValueError(f"TokenConstraint: {self.n_classes} classes, at most {MAX_CLASSES}")
        lo, hi = int(token_class.min()), int(token_class.max())
        if lo < 0 or hi >= self.n_classes:
            raise ValueError(f"TokenConstraint: token_class holds {lo if lo < 0 else hi}, outside [0, n_classes = {self.n_classes})")
        if int(trans.min()) < -1 or int(trans.max()) >= self.n_states:
            bad = int(trans.min()) if int(trans.min()) < -1 else int(trans.max())
            raise ValueError(f"TokenConstraint: trans holds {bad}, outside [-1, n_states = {self.n_states})")
        self.token_class, self.trans = token_class.contiguous(), trans.contiguous()
        # every state must allow at least one class that holds at least one token (HF raises when the function returns nothing)
        populated = torch.zeros(self.n_classes, dtype=torch.bool)
        populated[self.token_class.long()] = True
        empty = ~((self.trans >= 0) & populated[None]).any(dim=1)
        if bool(empty.any()):
            raise ValueError(f"TokenConstraint: state {int(empty.nonzero()[0])} allows no token")
        self.start = self.check_start("TokenConstraint", start)

    # ---- start states
    def check_start(self, who, state):
        if isinstance(state, bool) or not isinstance(state, numbers.Integral) or not 0 <= state < self.n_states:
            raise ValueError(f"{who}: a start state must be an int in [0, n_states = {self.n_states}), got {state!r}")
        return int(state)

    def starts(self, who, constraint_start, n_req, repeat=1):
        """``constraint_start`` of a generate entry -> int32 [n_req * repeat], request-major: None is the constraint's own start,
        one int serves every request, a list / tuple / 1-D tensor holds one per request (the rules and messages of the other
        per-request arguments)."""
        v = constraint_start
        if isinstance(v, torch.Tensor) and v.dim() >= 1:
            if v.dim() != 1:
                raise ValueError(f"{who}: constraint_start must be one value or a 1-D sequence, got a {v.dim()}-D tensor")
            v = v.tolist()
        if isinstance(v, (list, tuple)):
            if len(v) != n_req:
                raise ValueError(f"{who}: constraint_start has {len(v)} values for {n_req} requests")
            states = []
            for r, s in enumerate(v):
                if isinstance(s, bool) or not isinstance(s, numbers.Integral) or not 0 <= s < self.n_states:
                    raise ValueError(f"{who}: constraint_start[{r}] = {s!r} is not a state in [0, n_states = {self.n_states})")
                states.append(int(s))
        else:
            if isinstance(v, torch.Tensor):
                v = v.item()
            states = [self.start if v is None else self.check_start(f"{who}: constraint_start", v)] * n_req
        return torch.tensor([s for s in states for _ in range(repeat)], dtype=torch.int32)

    # ---- the rule on the host
    def allowed(self, state):
        """The token ids that ``state`` allows, ascending."""
        state = self.check_start("TokenConstraint.allowed", state)
        ok = self.trans[state] >= 0
        return ok[self.token_class.long()].nonzero()[:, 0].tolist()

    def next(self, state, token):
        """The state after ``token`` in ``state``, or -1 when the state does not allow it (or the id lies outside the vocabulary)."""
        token = int(token)
        if not 0 <= token < self.vocab:
            return -1
        return int(self.trans[state, int(self.token_class[token])])

    def walk(self, tokens, start=None):
        """-> (state, n_accepted): the automaton follows ``tokens`` from ``start`` (default: its own) while it allows them;
        n_accepted == len(tokens) when it allows them all, else the index of the first token that is not allowed and the state
        there."""
        state = self.start if start is None else self.check_start("TokenConstraint.walk", start)
        for i, t in enumerate(tokens):
            nxt = self.next(state, t)
            if nxt < 0:
                return state, i
            state = nxt
        return state, len(tokens)

    # ---- builders
    @staticmethod
    def _ids(who, vocab, ids):
        vocab = int(vocab)
        if vocab < 1:
            raise ValueError(f"{who}: vocab must be >= 1, got {vocab}")
        out = []
        for t in ids:
            if isinstance(t, bool) or not isinstance(t, numbers.Integral) or not 0 <= t < vocab:
                raise ValueError(f"{who}: token id {t!r} outside [0, vocab = {vocab})")
            out.append(int(t))
        return vocab, out

    @classmethod
    def from_allowed_tokens(cls, vocab, ids):
        """One state in which only ``ids`` are allowed, forever (an allowed vocabulary)."""
        vocab, ids = cls._ids("TokenConstraint.from_allowed_tokens", vocab, ids)
        token_class = torch.zeros(vocab, dtype=torch.int32)
        token_class[ids] = 1
        return cls(token_class, torch.tensor([[-1, 0]], dtype=torch.int32))

    @classmethod
    def from_suppressed_tokens(cls, vocab, ids):
        """One state in which every token but ``ids`` is allowed, forever (HF ``suppress_tokens``)."""
        vocab, ids = cls._ids("TokenConstraint.from_suppressed_tokens", vocab, ids)
        token_class = torch.zeros(vocab, dtype=torch.int32)
        token_class[ids] = 1
        return cls(token_class, torch.tensor([[0, -1]], dtype=torch.int32))

    @classmethod
    def free(cls, vocab):
        """One state that allows every token: the call computes what it computes without a constraint."""
        return cls.from_suppressed_tokens(vocab, [])

    @classmethod
    def from_sequences(cls, vocab, sequences, end_token):
        """A trie: the output is exactly one of ``sequences`` (lists of ids) followed by ``end_token``.  State 0 is the root; the
        last state is terminal: it allows ``end_token`` only and loops on it.  One sequence may be a prefix of another (the node
        then allows both the longer one's next token and ``end_token``); ``end_token`` may not occur inside a sequence."""
        who = "TokenConstraint.from_sequences"
        vocab, (end,) = cls._ids(who, vocab, [end_token])
        seqs = [cls._ids(who, vocab, s)[1] for s in sequences]
        if not seqs or any(not s for s in seqs):
            raise ValueError(f"{who}: needs at least one sequence, and every sequence at least one id")
        if any(end in s for s in seqs):
            raise ValueError(f"{who}: end_token {end} occurs inside a sequence")
        used = sorted({t for s in seqs for t in s} | {end})
        cls_of = {t: i + 1 for i, t in enumerate(used)}  # class 0: every token no sequence uses
        token_class = torch.zeros(vocab, dtype=torch.int32)
        for t, c in cls_of.items():
            token_class[t] = c
        nodes, ends_here = [{}], [False]  # the trie, children by token
        for s in seqs:
            at = 0
            for t in s:
                if t not in nodes[at]:
                    nodes[at][t] = len(nodes)
                    nodes.append({})
                    ends_here.append(False)
                at = nodes[at][t]
            ends_here[at] = True
        terminal = len(nodes)
        if terminal + 1 > MAX_STATES:
            raise ValueError(f"{who}: the trie has {terminal + 1} states, at most {MAX_STATES}")
        trans = torch.full((terminal + 1, len(used) + 1), -1, dtype=torch.int32)
        for i, kids in enumerate(nodes):
            for t, j in kids.items():
                trans[i, cls_of[t]] = j
            if ends_here[i]:
                trans[i, cls_of[end]] = terminal
        trans[terminal, cls_of[end]] = terminal
        return cls(token_class, trans)

    @classmethod
    def union(cls, constraints):
        """The automata side by side, with disjoint state ranges -> (combined, starts): member i's states are its own shifted by
        the number of states before it, and starts[i] is its start state there, so that different requests of one call can
        follow different forms (``constraint_start=[starts[form of r] for r ...]``).  The classes of the union are the distinct
        tuples of member classes."""
        cs = list(constraints)
        if not cs:
            raise ValueError("TokenConstraint.union: needs at least one constraint")
        if any(c.vocab != cs[0].vocab for c in cs):
            raise ValueError(f"TokenConstraint.union: the vocabularies differ ({[c.vocab for c in cs]})")
        joint = torch.stack([c.token_class for c in cs], dim=1)  # [V, members]
        tuples, token_class = torch.unique(joint, dim=0, return_inverse=True)
        n_states = sum(c.n_states for c in cs)
        if n_states > MAX_STATES:
            raise ValueError(f"TokenConstraint.union: {n_states} states, at most {MAX_STATES}")
        if tuples.shape[0] > MAX_CLASSES:
            raise ValueError(f"TokenConstraint.union: {tuples.shape[0]} classes, at most {MAX_CLASSES}")
        rows, starts, base = [], [], 0
        for i, c in enumerate(cs):
            t = c.trans[:, tuples[:, i].long()]  # [member states, union classes]
            rows.append(torch.where(t >= 0, t + base, t))
            starts.append(base + c.start)
            base += c.n_states
        return cls(token_class.to(torch.int32), torch.cat(rows).to(torch.int32), start=starts[0]), starts
