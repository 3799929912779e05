"""Streaming beam search (RNNTModel.beam_stream / beam_streams -> rnnt_engine_beam_stream_push) against the offline
RNNTModel.beam_search of the same frames, in one process: the weights of the decode_ref_widths fixture (tests/helpers.py DECODE_CASES:
ConvPredictor E = 512, O = H = V = 1024, the reference's config/basic_sp_convjs_fullcausal.yaml widths), T = 1000 seeded N(0,1) frames,
beam 4, max_length 200, 10 symbols per frame.

Reported: beam_search offline (this tool's own measurement, every run); one stream fed in pushes of 1000, 50, 10 and 1 frames — the whole
utterance's time and the median and worst time of a push (host clock around push_encoded, which ends in the push's synchronisation) —
and groups of 8 and 32 streams (different utterances) in 50-frame pushes, per stream.  Every streamed result is compared with the
offline one.  Medians of --reps repetitions after a warm-up.  Writes --out (default profiles/beam_stream_bench.txt)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rnnt_amd  # noqa: E402
from tests.helpers import load_decode_case  # noqa: E402


class Enc(torch.nn.Module):
    def forward(self, x):
        return x  # (1, H, T) already

    def calc_output_lens(self, lens):
        return lens


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--max-length", type=int, default=200)
    ap.add_argument("--chunks", default="1000,50,10,1")
    ap.add_argument("--groups", default="8,32")
    ap.add_argument("--group-chunk", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_stream_bench.txt"))
    a = ap.parse_args()
    c = load_decode_case(os.path.join(ROOT, "tests", "golden"), "decode_ref_widths")
    spec = c["spec"]
    pred = rnnt_amd.ConvPredictor(spec["V"], spec["O"], spec["E"], 0.3)
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    for mod, sd in ((pred, c["pred_sd"]), (joint, c["joint_sd"])):
        mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model = rnnt_amd.RNNTModel(pred, Enc(), joint).cuda().eval()
    T, H = a.T, spec["H"]
    groups = [int(g) for g in a.groups.split(",")]
    rng = np.random.default_rng(1)
    mels = [torch.from_numpy(rng.standard_normal((1, H, T)).astype(np.float32)).cuda() for _ in range(max(groups + [1]))]
    lens = torch.tensor([T], device="cuda")
    kw = dict(beam_size=a.beam, max_length=a.max_length)
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    want = [model.beam_search(mel, lens, return_nbest=True, **kw) for mel in mels]  # (warms the offline search up too)
    off = [clock(lambda: model.beam_search(mels[0], lens, return_nbest=True, **kw))[0] for _ in range(a.reps)]
    t_off = statistics.median(off)
    say(f"streaming beam search: decode_ref_widths weights (E={spec['E']} O={spec['O']} H={H} V={spec['V']}), T={T} N(0,1) frames, beam {a.beam}, "
        f"max_length {a.max_length}, 10 symbols per frame; best hypothesis {len(want[0][0][0])} labels; medians of {a.reps} repetitions after "
        f"a warm-up ({torch.cuda.get_device_name()})")
    say(f"offline beam_search: {t_off * 1e3:.2f} ms (min {min(off) * 1e3:.2f}, max {max(off) * 1e3:.2f})")
    say(f"{'push':>6} {'pushes':>6} {'stream ms':>10} {'x offline':>9} {'median push ms':>15} {'worst push ms':>14}  result")
    for k in (int(x) for x in a.chunks.split(",")):
        def stream():
            s = model.beam_stream(**kw)
            lat = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, T, k):
                p0 = time.perf_counter()
                s.push_encoded(mels[0][..., i:i + k])
                lat.append(time.perf_counter() - p0)
            return time.perf_counter() - t0, lat, s.nbest, s.last_path

        stream()
        res = sorted((stream() for _ in range(a.reps)), key=lambda r: r[0])
        total, lat, _, path = res[a.reps // 2]
        same = "equal to offline" if all(r[2] == want[0] for r in res) else "DIFFERS from offline"
        say(f"{k:6d} {len(lat):6d} {total * 1e3:10.2f} {total / t_off:9.2f} {statistics.median(lat) * 1e3:15.3f} {max(lat) * 1e3:14.3f}  {same} ({path})")
    k = a.group_chunk
    for n in groups:
        def group():
            g = model.beam_streams(n, **kw)
            lat = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, T, k):
                p0 = time.perf_counter()
                g.push_encoded([mel[..., i:i + k] for mel in mels[:n]])
                lat.append(time.perf_counter() - p0)
            return time.perf_counter() - t0, lat, g.nbest

        group()
        res = sorted((group() for _ in range(a.reps)), key=lambda r: r[0])
        total, lat, _ = res[a.reps // 2]
        same = "equal to offline" if all(r[2] == want[:n] for r in res) else "DIFFERS from offline"
        say(f"group of {n:2d} streams, {k}-frame pushes: {total * 1e3:9.2f} ms = {total / n * 1e3:7.2f} ms per stream ({total / n / t_off:.2f} x offline); "
            f"push median {statistics.median(lat) * 1e3:.3f} ms, worst {max(lat) * 1e3:.3f} ms; every stream {same}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
