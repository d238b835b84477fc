"""The argument checks of closed-loop variable-rate calls: the ladder and the token bucket, as ``encode_vbr`` and a vbr streaming
session take them.  Plain arithmetic - no torch, no library."""
import ctypes

_MAX_RUNGS = 8                   # VBR_MAX_RUNGS of the library
_Q8 = 256                        # the token bucket of a capped closed-loop call counts 1/256 bit
_I32_MAX = 2 ** 31 - 1


def _check_ladder(ladder, z_dim, var_bit):
    """The ladder of a closed-loop call as a ctypes int32 array, or ValueError: 1 to 8 integer bit counts in [0, z_dim], strictly
    ascending, on a variable-rate model."""
    if not var_bit:
        raise ValueError("encode_vbr: a fixed-rate model (var_bit = false) has no bit mask to choose")
    rungs = [int(n) for n in ladder]
    if any(float(a) != float(b) for a, b in zip(rungs, ladder)):
        raise ValueError(f"encode_vbr: the rungs must be integer bit counts, got {list(ladder)}")
    if not 1 <= len(rungs) <= _MAX_RUNGS:
        raise ValueError(f"encode_vbr: the ladder takes 1 to {_MAX_RUNGS} rungs, got {len(rungs)}: {rungs}")
    if any(n < 0 or n > z_dim for n in rungs) or any(b <= a for a, b in zip(rungs, rungs[1:])):
        raise ValueError(f"encode_vbr: the rungs must lie in [0, {z_dim}] and ascend strictly, got {rungs}")
    return (ctypes.c_int32 * len(rungs))(*rungs), len(rungs)


def _check_cap_q8(rungs, rate_q8, burst_q8):
    """The bucket of a capped closed-loop call as two ints, or ValueError (what the library refuses with BVC_EINVAL): neither negative,
    both int32, and a full bucket holds rung 0."""
    if rate_q8 is None or burst_q8 is None:
        raise ValueError("encode_vbr: a rate cap takes both rate_q8 and burst_q8")
    if int(rate_q8) != rate_q8 or int(burst_q8) != burst_q8:
        raise ValueError(f"encode_vbr: rate_q8 and burst_q8 are integers (1/256 bit), got {rate_q8!r}, {burst_q8!r}")
    rate_q8, burst_q8 = int(rate_q8), int(burst_q8)
    if rate_q8 < 0 or burst_q8 < 0 or rate_q8 > _I32_MAX or burst_q8 > _I32_MAX:
        raise ValueError(f"encode_vbr: rate_q8 = {rate_q8} and burst_q8 = {burst_q8} must lie in [0, 2^31)")
    if burst_q8 < int(rungs[0]) * _Q8:
        raise ValueError(f"encode_vbr: a bucket of {burst_q8 / _Q8:g} bits never holds rung 0 ({int(rungs[0])} bits)")
    return rate_q8, burst_q8


def cap_q8(conf, rungs, rate_cap, burst):
    """``rate_cap`` [bit/s] and ``burst`` [bits] of a capped closed-loop call as (rate_q8, burst_q8), None without a cap; ValueError as
    ``_check_cap_q8``.  rate_q8 = round(rate_cap * hopsize / fs * 256), burst_q8 = round(burst * 256), the default burst four times the
    top rung."""
    if rate_cap is None:
        if burst is not None:
            raise ValueError("encode_vbr: burst without rate_cap")
        return None
    if not (rate_cap >= 0) or (burst is not None and not (burst >= 0)) or rate_cap == float("inf") or burst == float("inf"):
        raise ValueError(f"encode_vbr: rate_cap = {rate_cap} and burst = {burst} must be finite and not negative")
    if burst is None:
        burst = 4 * int(rungs[-1])
    return _check_cap_q8(rungs, round(rate_cap * conf["hopsize"] / conf["fs"] * _Q8), round(burst * _Q8))
