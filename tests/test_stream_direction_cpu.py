"""Host arithmetic of the directed streaming sessions (no GPU): which frames a finished stream still gets and in which ticks, and
the layout of a packet."""
import numpy as np
import pytest

FRAME, PAD, NFFT = 256, 256, 1024
RPAD = NFFT - FRAME - PAD                                     # right reflect padding: 512 samples


def simulate_stream(hop, t_open, t_fin, n_last, ticks):
    """One row of a session, tick by tick, from the library's own rules: the session's fill level (as in tests/test_stream_slots_cpu.py),
    the stream's sample 0 at session sample 256 * frame0, its samples arriving one hop per tick from tick t_open on; from tick t_fin on
    all n samples and the 512 samples of padding behind them are there.  A session frame is the stream's frame i = f - frame0; it is the
    stream's own only if every sample it reads ([256 i - 256, 256 i + 768) of the stream, padding included) is there when the tick runs.
    Returns (n, frames the stream got before tick t_fin, {tick: frames of the stream in that tick} from t_fin on, the tick after which
    every frame below n // 256 is out)."""
    from bvcodec.streaming import join_plan
    delay, frame0, _ = join_plan(t_open * hop, hop)
    n = (t_fin - t_open) * hop + n_last
    total = n // FRAME
    fill, emitted = PAD, 0
    before, per_tick, done_tick = 0, {}, None
    for t in range(ticks):
        fill += hop
        k = (fill - NFFT) // FRAME + 1 if fill >= NFFT else 0
        # what the row holds of the stream when this tick's front-end runs
        have = (t - t_open + 1) * hop if t < t_fin else n + RPAD
        mine = 0
        for f in range(emitted, emitted + k):
            i = f - frame0
            if t >= t_open and 0 <= i < total:
                assert FRAME * i + NFFT - PAD <= have, (hop, t_open, t_fin, n_last, t, i)     # never a frame ahead of its samples
                mine += 1
        if t < t_fin:
            before += mine
        elif done_tick is None:
            per_tick[t] = mine
        emitted += k
        fill -= FRAME * k
        if done_tick is None and t >= t_fin and emitted >= frame0 + total:
            done_tick = t
    return n, before, per_tick, done_tick


@pytest.mark.parametrize("hop", [300, 441, 700, 1100])
def test_finish_plan_against_simulated_schedule(hop):
    """n over every residue mod 256 (by the choice of n_last and of the stream's life), every joining tick 0 .. 60."""
    from bvcodec.streaming import finish_plan
    residues = set()
    for t_open in range(0, 61):
        for life, n_last in [(3, 0), (3, hop), (4, 1), (7, hop - 1), (5, (t_open * 37) % (hop + 1)), (9, (t_open * 101 + 13) % (hop + 1))]:
            t_fin = t_open + life
            n, total, plan = finish_plan(t_open, t_fin, n_last, hop)
            sn, before, per_tick, done_tick = simulate_stream(hop, t_open, t_fin, n_last, t_fin + 12)
            assert n == sn and total == n // FRAME
            assert done_tick is not None
            assert plan == sorted(per_tick.items()), (t_open, life, n_last)
            assert plan[0][0] == t_fin and plan[-1][0] == done_tick
            assert before + sum(c for _, c in plan) == total                  # ALL frames of the offline call
            assert sum(c for _, c in plan) >= 2                               # ... of which a close would have left at least two out
            residues.add(n % FRAME)
    # the sweep above does not reach every residue for every hop: the rest, from one joining tick
    for r in range(FRAME):
        if r in residues:
            continue
        for life in range(3, 3 + FRAME):
            n_last = (r - life * hop) % FRAME
            if n_last <= hop:
                break
        n, total, plan = finish_plan(17, 17 + life, n_last, hop)
        assert n % FRAME == r
        sn, before, per_tick, done_tick = simulate_stream(hop, 17, 17 + life, n_last, 17 + life + 12)
        assert (n, plan) == (sn, sorted(per_tick.items())) and before + sum(c for _, c in plan) == total
        residues.add(r)
    assert residues == set(range(FRAME))


def test_finish_plan_refuses_what_the_library_refuses():
    from bvcodec.streaming import finish_plan
    with pytest.raises(ValueError):
        finish_plan(0, 1, 71, 441)                                            # n = 512: too short for the padding
    assert finish_plan(0, 1, 72, 441)[:2] == (513, 2)
    with pytest.raises(ValueError):
        finish_plan(0, 5, 442, 441)
    with pytest.raises(ValueError):
        finish_plan(0, 5, -1, 441)


@pytest.mark.parametrize("z", [64, 26, 8, 70, 16, 48, 96, 128, 144])
def test_packet_layout_against_packbits(z):
    """A frame on the wire: ceil(z / 8) bytes for every row; a row with nbits active bits uses the first ceil(nbits / 8) of them, bit i
    in byte i // 8 at position i % 8 - numpy's little bit order - and everything behind nbits is 0."""
    rng = np.random.default_rng(z)
    bpf = -(-z // 8)
    assert bpf == (z + 7) // 8
    for nbits in sorted({0, 1, 7, 8, 9, 17, 26, 35, z - 1, z} & set(range(z + 1))):
        bits = rng.integers(0, 2, size=(5, z)).astype(np.uint8)
        frame = np.zeros((5, bpf), np.uint8)
        for i in range(nbits):                                                # the definition, bit by bit
            frame[:, i // 8] |= bits[:, i] << (i % 8)
        used = -(-nbits // 8)
        want = np.packbits(bits[:, :nbits], axis=1, bitorder="little")
        assert want.shape[1] == used
        assert np.array_equal(frame[:, :used], want) and not frame[:, used:].any()
        back = np.unpackbits(frame, axis=1, bitorder="little")[:, :z]
        assert np.array_equal(back[:, :nbits], bits[:, :nbits]) and not back[:, nbits:].any()


def test_bytes_used_per_rate_of_the_shipped_config():
    """The bit counts behind the rates the GPU tests use (bits per frame = round(rate * 256 / 22050), at most z_dim = 64)."""
    from bvcodec import config
    conf = config.load_config(config.DEFAULT_CONFIG)
    z = conf["z_dim"]
    assert -(-z // 8) == 8
    for rate, nbits, used in ((1500, 17, 3), (2200, 26, 4), (3000, 35, 5), (6000, 64, 8)):
        got = int(min(z, np.round(rate * conf["hopsize"] / conf["fs"])))
        assert got == nbits and -(-got // 8) == used
