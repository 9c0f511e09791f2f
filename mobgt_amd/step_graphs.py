"""The captured hipGraphs of one `train.TrainStep`, in ONE cache with one lifetime: `recapture()` clears it, everything else only
adds.  An entry is `(graphs, loss)`: the graphs replayed in order (one for most forms; phase A + the parts of phase B for the
overlap form) and the static tensor their capture left the loss in (None for an entry without a forward pass).  A key says what
the entry RUNS, never where it was captured:

    ("step", batch, comm)      one step of that batch; comm: the gradient exchange is a node of the graph
    ("micro", batch)           one micro-step of an accumulation window
    ("update", comm)           the update that ends a window
    ("opt",)                   AdamW alone (the forms that exchange between two replays)
    ("group", batches, comm)   the steps of those batches, in that order, as one graph (`group_key`)

Imports nothing from the package, needs no torch (like step_state.py)."""
from collections import namedtuple

Entry = namedtuple("Entry", "graphs loss")


def group_key(i, k, nb, comm):
    """Key of steps i .. i + k - 1 over a cyclic pool of nb batches: the batch indices THEMSELVES, so a pool that grows later
    (`TrainStep.add_batch`) cannot make a cached group mean other batches."""
    return ("group", tuple((i + j) % nb for j in range(k)), bool(comm))


class StepGraphs:
    def __init__(self):
        self._entries = {}

    def get(self, key, capture, *args):
        """The entry under `key`; a key seen for the first time is captured now: `capture(*args)` -> Entry."""
        e = self._entries.get(key)
        if e is None:
            e = self._entries[key] = capture(*args)
        return e

    def of(self, kind):
        """{key: entry} of one kind ("step", "micro", "update", "opt", "group")."""
        return {k: e for k, e in self._entries.items() if k[0] == kind}

    def clear(self):
        self._entries.clear()
