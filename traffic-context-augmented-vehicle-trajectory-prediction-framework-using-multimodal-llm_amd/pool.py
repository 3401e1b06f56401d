"""Slot bookkeeping of LlamaMultiModal.generate_pool: which request runs in which decode slot.  Host logic only -- no torch, no
device -- so that it can be driven by a scripted `finished` feed."""


class SlotScheduler:
    """R requests are served exactly once, first in first out, by a fixed pool of decode slots.  The caller alternates
    ``admissions()`` (prefill each returned request into its slot), some decode steps, and ``retire(finished)`` with the
    device's per-slot finished flags, until ``busy()`` is false.
    ``group`` = G > 1: admissions come in groups of fixed width (``admission_groups()``): a group is released only when
    min(G, waiting requests) slots are free, so that every admission pass of the caller has the same shape."""

    def __init__(self, n_requests, slots, group=1):
        if slots < 1 or n_requests < 0:
            raise ValueError("SlotScheduler: slots >= 1 and n_requests >= 0 required")
        if not 1 <= int(group) <= int(slots):
            raise ValueError(f"SlotScheduler: group = {group} must be in [1, slots = {slots}]")
        self.n_requests, self.slots, self.group = int(n_requests), int(slots), int(group)
        self.slot_request = [None] * self.slots  # the live request of every slot
        self.next_request = 0
        self.retired = []  # (request, slot) in the order they ended

    def admissions(self):
        """-> [(slot, request)]: the next requests of the queue, one per free slot (lowest slot first); the slots are taken."""
        out = []
        for s in range(self.slots):
            if self.next_request == self.n_requests:
                break
            if self.slot_request[s] is None:
                self.slot_request[s] = self.next_request
                out.append((s, self.next_request))
                self.next_request += 1
        return out

    def admission_groups(self):
        """-> [[(slot, request), ...], ...]: groups of up to ``group`` pairs, first in first out, lowest free slots first; the
        slots are taken.  A group is released only while free slots >= min(group, waiting requests): at the start
        slots // group full groups go at once, a free slot then waits for group - 1 others (or for the queue to be shorter
        than the group), and the tail goes as soon as there is room for all of it.  group = 1: admissions(), one pair per group."""
        out = []
        while self.next_request < self.n_requests:
            need = min(self.group, self.n_requests - self.next_request)
            free = [s for s in range(self.slots) if self.slot_request[s] is None]
            if len(free) < need:
                break
            g = []
            for s in free[:need]:
                self.slot_request[s] = self.next_request
                g.append((s, self.next_request))
                self.next_request += 1
            out.append(g)
        return out

    def retire(self, finished):
        """finished: one flag per slot, as read from the device.  Frees the slots whose live request has ended (a flag on a
        slot that holds no request -- an idle slot -- means nothing) and returns those requests."""
        if len(finished) != self.slots:
            raise ValueError("SlotScheduler.retire: one flag per slot")
        out = []
        for s, f in enumerate(finished):
            r = self.slot_request[s]
            if r is not None and f:
                self.slot_request[s] = None
                self.retired.append((r, s))
                out.append(r)
        return out

    def live(self):
        return sum(r is not None for r in self.slot_request)

    def busy(self):
        """True while a request is live or waiting."""
        return self.next_request < self.n_requests or self.live() > 0
