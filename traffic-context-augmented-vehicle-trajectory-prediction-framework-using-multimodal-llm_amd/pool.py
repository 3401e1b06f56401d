"""Slot bookkeeping of LlamaMultiModal.generate_pool: which request runs in which decode slot.  Host logic only -- no torch, no
device -- so that it can be driven by a scripted `finished` feed."""


class SlotScheduler:
    """R requests are served exactly once, first in first out, by a fixed pool of decode slots.  The caller alternates
    ``admissions()`` (prefill each returned request into its slot), some decode steps, and ``retire(finished)`` with the
    device's per-slot finished flags, until ``busy()`` is false."""

    def __init__(self, n_requests, slots):
        if slots < 1 or n_requests < 0:
            raise ValueError("SlotScheduler: slots >= 1 and n_requests >= 0 required")
        self.n_requests, self.slots = int(n_requests), int(slots)
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
