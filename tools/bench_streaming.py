#!/usr/bin/env python3
"""BASELINE.json configs[4]: 256 concurrent streams, 20 ms (441-sample) hops, config_varBitRate @ 3 kbit/s,
per-hop encode+decode on one MI355X.  Prints one JSON line with p50 / p99 per-hop latency.

--churn [--ticks N]: the same session with streams that come and go: every 10th tick (5 times per second of audio) one slot is
closed and another opened at a bitrate of its own, and every 250th tick 32 slots are closed and re-opened at once.  Reports the
ticks in which nothing changes ("steady"), the ticks that carry a close / open to the device ("update") and the ticks in which
streams start ("join": per-row reset of the GRU states, the generator histories and the reflect padding) separately.

--direction send|recv|duplex [--loss P]: the same 256 streams and inputs through a session that runs one half (send: samples ->
packets; recv: packets -> samples) or both (duplex, the default run's loopback tick).  recv replays the packets of a send run
(not timed) in ticks of the frame counts that run emitted; --loss P marks a seeded share P of the frames as not arrived;
--conceal none|prior (recv only): what the session does with them (none: frames of no bits; prior: generated from the prior net);
--repair W (recv only): the session keeps a repair window of W frames (no packet arrives late: what the window itself costs a tick).

--late P [--delay D] [--repair W] [--conceal none|prior]: a receive session with a repair window (default 16 frames) in which a seeded
share P of the frames is pushed as not arrived and handed in with ``late`` D ticks afterwards (default 2).  A tick's time includes
its ``late`` calls.  Reports the ticks that repair nothing ("steady") and those that replay ("repair") separately, with the passes
(groups of rows that replay from the same tick) per repair tick."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np, torch
from gpu_common import make_model
from bvcodec import synth
from bvcodec.streaming import StreamingCodec, StreamingDecoder, StreamingEncoder

B, hop, hops = 256, 441, 300


def churn():
    import random
    from bvcodec.streaming import join_plan
    ticks = int(sys.argv[sys.argv.index("--ticks") + 1]) if "--ticks" in sys.argv else 1500
    model = make_model()[0]
    x = synth.synthetic_speech(B, hop * 300, seed=3, kind="noise").to("cuda:0")
    sc = StreamingCodec(model, B, 3000, hop=hop)
    rng = random.Random(1)
    idle = set(range(200, B))
    for b in idle:
        sc.close(b)
    kind, lat, joins_at = {}, [], {}
    for t in range(ticks):
        n = 32 if t % 250 == 125 else (1 if t % 10 == 0 else 0)
        if t >= 60 and n:
            kind[t] = "update"
            for _ in range(n):
                b = rng.choice(sorted(set(range(B)) - idle))
                sc.close(b)
                o = rng.choice(sorted(idle))
                sc.open(o, rng.choice((1500, 3000, 6000)))
                idle.discard(o); idle.add(b)
            jt = join_plan(t * hop, hop)[2]
            joins_at[jt] = joins_at.get(jt, 0) + n
        i = t % 300
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c, w = sc.push(x[:, i * hop:(i + 1) * hop])
        torch.cuda.synchronize(); lat.append((time.perf_counter() - t0) * 1e3)
    model.check_status()
    lat = np.array(lat)
    rows = {"steady": [], "update": [], "join_1": [], "join_32": []}
    for t in range(60, ticks):
        if t in joins_at:
            rows["join_32" if joins_at[t] >= 32 else "join_1"].append(lat[t])      # (a join tick that also carries an update counts as a join)
        elif t in kind:
            rows["update"].append(lat[t])
        else:
            rows["steady"].append(lat[t])
    out = {"config": f"configs[4] with churn: {B} slots ({B - len(idle)} open) x 20 ms hops, {ticks} ticks; one close + open every 10th tick, 32 at once every 250th",
           "hop_budget_ms": 20.0}
    for k, v in rows.items():
        if v:
            v = np.array(v)
            out[k] = {"ticks": int(v.size), "p50_ms": round(float(np.percentile(v, 50)), 3), "p99_ms": round(float(np.percentile(v, 99)), 3),
                      "max_ms": round(float(v.max()), 3)}
    print(json.dumps(out))


def argval(name, default, cast):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def late():
    share, delay, W = argval("--late", 0.01, float), argval("--delay", 2, int), argval("--repair", 16, int)
    conceal = argval("--conceal", "none", str)
    model = make_model()[0]
    x = synth.synthetic_speech(B, hop * hops, seed=3, kind="noise").to("cuda:0")
    tx = StreamingCodec(model, B, 3000, hop=hop, direction="send")
    sent = [tx.push(x[:, i * hop:(i + 1) * hop])[0].clone() for i in range(hops)]
    sent = [p for p in sent if p.shape[1]]
    del tx
    g = torch.Generator().manual_seed(11)
    lost = [torch.rand(B, p.shape[1], generator=g) < share for p in sent]
    first = np.cumsum([0] + [p.shape[1] for p in sent])
    host = [p.cpu().numpy() for p in sent]
    sc = StreamingCodec(model, B, 3000, direction="recv", conceal=conceal, repair=W)
    lat, passes, rows, taken, asked = [], [], [], 0, 0
    for t, (p, lo) in enumerate(zip(sent, lost)):
        due = lost[t - delay].nonzero().tolist() if t >= delay else []
        present = (~lo).to(torch.uint8).to("cuda:0")
        torch.cuda.synchronize(); t0 = time.perf_counter()
        got = [sc.late(b, int(first[t - delay]) + j, host[t - delay][b, j].tobytes()) for b, j in due]
        sc.push_packets(p, present)
        torch.cuda.synchronize(); lat.append((time.perf_counter() - t0) * 1e3)
        asked += len(due); taken += sum(got)
        passes.append(1 if any(got) else 0)                 # the frames of ONE earlier tick: their rows start together
        rows.append(len({b for (b, j), ok in zip(due, got) if ok}))
    model.check_status()
    lat, passes, rows = np.array(lat[50:]), np.array(passes[50:]), np.array(rows[50:])
    out = {"config": f"BASELINE configs[4]: {B} streams x 20 ms hops @ 3 kbit/s, recv session, repair window {W} frames, "
                     f"{share:.0%} of the frames {delay} ticks late", "conceal": conceal, "late_taken": taken, "late_handed_in": asked,
           "hop_budget_ms": 20.0}
    for name, sel in (("steady", passes == 0), ("repair", passes > 0)):
        if sel.any():
            v = lat[sel]
            out[name] = {"ticks": int(v.size), "p50_ms": round(float(np.percentile(v, 50)), 3), "p99_ms": round(float(np.percentile(v, 99)), 3),
                         "max_ms": round(float(v.max()), 3)}
    if (passes > 0).any():
        out["passes_per_repair_tick"] = round(float(passes[passes > 0].mean()), 2)
        out["rows_per_repair_tick"] = round(float(rows[passes > 0].mean()), 1)
    print(json.dumps(out))


def direction(which):
    loss = float(sys.argv[sys.argv.index("--loss") + 1]) if "--loss" in sys.argv else 0.0
    conceal = sys.argv[sys.argv.index("--conceal") + 1] if "--conceal" in sys.argv else None
    repair = argval("--repair", 0, int)
    if (conceal is not None or repair) and which != "recv":
        sys.exit("--conceal and --repair belong to --direction recv")
    model = make_model()[0]
    x = synth.synthetic_speech(B, hop * hops, seed=3, kind="noise").to("cuda:0")
    lat, frames = [], 0
    if which == "recv":
        tx = StreamingCodec(model, B, 3000, hop=hop, direction="send")
        sent = [tx.push(x[:, i * hop:(i + 1) * hop])[0].clone() for i in range(hops)]
        sent = [p for p in sent if p.shape[1]]
        del tx
        g = torch.Generator().manual_seed(11)
        present = [(torch.rand(B, p.shape[1], generator=g) >= loss).to(torch.uint8).to("cuda:0") for p in sent]
        sc = StreamingCodec(model, B, 3000, direction="recv", repair=repair, **({} if conceal is None else {"conceal": conceal}))
        for p, pr in zip(sent, present):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            sc.push_packets(p, pr)
            torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
            frames += p.shape[1]
        lost = 1.0 - float(torch.cat([pr.float().flatten() for pr in present]).mean())
    else:
        sc = StreamingCodec(model, B, 3000, hop=hop, direction=which)
        for i in range(hops):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            a, _ = sc.push(x[:, i * hop:(i + 1) * hop])
            torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
            frames += a.shape[1]
        lost = 0.0
    model.check_status()
    n = len(lat)
    lat = np.array(lat[50:]) * 1e3
    print(json.dumps({"config": f"BASELINE configs[4]: {B} streams x 20 ms hops @ 3 kbit/s, {which} session",
                      "direction": which, "conceal": conceal, "repair": repair, "ticks": n, "timed_ticks": int(lat.size), "frames_lost": round(lost, 4),
                      "p50_ms": round(float(np.percentile(lat, 50)), 3), "p99_ms": round(float(np.percentile(lat, 99)), 3),
                      "mean_ms": round(float(lat.mean()), 3), "hop_budget_ms": 20.0, "frames_per_tick": round(frames / n, 3)}))


if "--churn" in sys.argv:
    churn()
    sys.exit(0)
if "--late" in sys.argv:
    late()
    sys.exit(0)
if "--direction" in sys.argv:
    which = sys.argv[sys.argv.index("--direction") + 1]
    if which not in ("send", "recv", "duplex"):
        sys.exit("--direction send|recv|duplex")
    direction(which)
    sys.exit(0)
incremental = "--context" not in sys.argv      # --context: stateless vocoder that re-runs a 26-frame context per hop
python_path = "--python" in sys.argv or not incremental     # --python: the round-1 per-hop schedule driven from Python
model = make_model()[0]
x = synth.synthetic_speech(B, hop * hops, seed=3, kind="noise").to("cuda:0")
lat, frames = [], 0
if python_path:
    enc, dec = StreamingEncoder(model, B, 3000), StreamingDecoder(model, B, incremental=incremental)
    for i in range(hops):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c = enc.push(x[:, i * hop:(i + 1) * hop])
        w = dec.push(c)
        torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
        frames += c.shape[1]
else:                                          # default: one library call per hop, replayed from a hipGraph once warm
    sc = StreamingCodec(model, B, 3000, hop=hop)
    for i in range(hops):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        c, w = sc.push(x[:, i * hop:(i + 1) * hop])
        torch.cuda.synchronize(); lat.append(time.perf_counter() - t0)
        frames += c.shape[1]
    model.check_status()
lat = np.array(lat[50:]) * 1e3
print(json.dumps({"config": "BASELINE configs[4]: 256 streams x 20 ms hops @ 3 kbit/s, per-hop encode+decode",
                  "schedule": "python-driven hop (round 1)" if python_path else ("bvc_stream_codec_tick: whole hop in one call, persistent recurrence" if os.environ.get("BVC_STREAM_FLOW") != "0" else ("bvc_stream_codec_tick: launch-per-layer recurrence, hipGraph-replayed" if os.environ.get("BVC_STREAM_NO_GRAPH") != "1" else "bvc_stream_codec_tick: launch-per-layer recurrence, eager launches")),
                  "vocoder": "incremental (history buffers)" if incremental else "context recompute (26 frames)",
                  "p50_ms": round(float(np.percentile(lat, 50)), 3), "p99_ms": round(float(np.percentile(lat, 99)), 3),
                  "mean_ms": round(float(lat.mean()), 3), "hop_budget_ms": 20.0, "frames_per_hop": round(frames / hops, 3),
                  "real_time_factor_per_stream": round(20.0 / float(lat.mean()), 2)}))
