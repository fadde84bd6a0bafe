"""The schedule of the refilled-slot formula decode (rd_formula_decode_stream), restated on the host, and the helpers its tests share.

The rule (csrc/formula_decoder.hip, dec_stream_admit_kernel): `slots` decode rows; formulas 0 .. min(N, slots) - 1 start in slots of the same
number.  A formula of `lens[i]` columns (start token and EOS included; max_new + 1 at the cap) is live for lens[i] - 1 steps.  At the end of
the step in which formulas finish, the finished slots take the waiting formulas: the lowest slot the lowest formula; a finished slot for
which nothing waits goes idle (-1) and stays idle."""
import numpy as np


def simulate(lens, slots):
    """int32 [steps][slots][2]: (formula, position) of every slot at the start of every step until the last formula has ended; an idle
    slot is (-1, its last position value, which is 0)."""
    lens = [int(v) for v in lens]
    assert slots >= 1 and len(lens) >= 1 and all(v >= 2 for v in lens)
    N = len(lens)
    src = [s if s < N else -1 for s in range(slots)]
    pos = [0] * slots
    nxt = min(N, slots)
    out = []
    while any(s >= 0 for s in src):
        out.append([[src[s], pos[s]] for s in range(slots)])
        done = []
        for s in range(slots):
            if src[s] < 0:
                continue
            pos[s] += 1
            if pos[s] == lens[src[s]] - 1:
                done.append(s)
        for s in done:                          # slot order
            pos[s] = 0
            if nxt < N:
                src[s] = nxt
                nxt += 1
            else:
                src[s] = -1
    return np.asarray(out, dtype=np.int32).reshape(len(out), slots, 2)


def refill_bound(lens, slots, look_ahead=0):
    """List scheduling (Graham): no slot idles while a formula waits, so the last formula to end started no later than
    floor(sum of the others / slots) and the schedule ends within floor(sum / slots) + max steps; `look_ahead`: what the host loop may run on."""
    work = [int(v) - 1 for v in lens]
    return sum(work) // slots + max(work) + look_ahead


def chunk_steps(lens, chunk):
    """Steps of the batch-synchronous path on the same formulas: every chunk runs as long as its longest formula."""
    work = [int(v) - 1 for v in lens]
    return sum(max(work[i: i + chunk]) for i in range(0, len(work), chunk))


def lens_of(ids, max_new):
    """Columns that count per row of batch-path ids [B][n_cols]: the first EOS's position plus one, or max_new + 1."""
    out = []
    for row in np.asarray(ids):
        eos = np.nonzero(row[1:] == 2)[0]
        out.append(int(eos[0]) + 2 if len(eos) else max_new + 1)
    return np.asarray(out, dtype=np.int32)
