"""Event timing shared by the measurement-update cost tools (aux_update_cost.py, standstill_cost.py, fix_cost.py, fix_past_cost.py)."""


def timed(h, st, x, P, call, warmup, launches):
    """microseconds of device time per call(): HIP events on the handle's filter stream `st` (a torch.cuda.ExternalStream) around `launches`
    calls behind `warmup` warm-up calls, the state set to (x, P) in front of each of the two runs"""
    import torch
    h.set_state(x, P)
    for _ in range(warmup):
        call()
    h.set_state(x, P)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(launches):
        call()
    e1.record(st)
    h.sync()
    return 1e3 * e0.elapsed_time(e1) / launches
