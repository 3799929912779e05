"""Streaming greedy decode (RNNTModel.greedy_stream) against offline greedy_decode on the same frames: one synthetic
1000-frame utterance with ~200 labels, the reference's widths (config/basic_sp_convjs_fullcausal.yaml: E=512, O=H=1024, V=1024, no
joint projections), built like tools/bench_decode.py.  Per chunk size: per-push wall latency p50 / p95 (host clock around push_encoded,
which ends in its synchronisation), the whole streamed utterance against the offline decode, and the paths that served the pushes.
Writes profiles/stream_decode_bench.txt."""
import collections
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rnnt_amd  # noqa: E402

T, H, V, E = 1000, 1024, 1024, 512
CHUNKS = (1, 4, 10, 16, 50, 1000)
REPS = 3


class Enc(torch.nn.Module):
    def forward(self, x):
        return x  # (1, H, T) already

    def calc_output_lens(self, lens):
        return lens


def main():
    torch.manual_seed(0)
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(V, H, E, 0.3), Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda().eval()
    mel = torch.randn(1, H, T, generator=torch.Generator().manual_seed(1)).cuda()
    lens = torch.tensor([T], device="cuda")
    ml = T * 10 + 2  # = unbounded for this utterance; the streams run with max_length=None
    # the blank logit's offset: bisected until the utterance decodes to about 200 labels (BASELINE's T/U of 5 frames per label)
    b0 = model.joint.joint_ln.bias[V - 1].item()
    lo, hi = 0.0, 4.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        with torch.no_grad():
            model.joint.joint_ln.bias[V - 1] = b0 + mid
        n = len(model.greedy_decode(mel, lens, max_length=ml))
        if abs(n - 200) <= 20:
            break
        lo, hi = (mid, hi) if n > 200 else (lo, mid)

    def offline():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.greedy_decode(mel, lens, max_length=ml)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    offline()
    runs = [offline() for _ in range(REPS)]
    t_off = sorted(r[0] for r in runs)[REPS // 2]
    want = runs[0][1]
    lines = [f"streaming greedy decode, T={T} frames, E={E} O=H={H} V={V}, blank bias +{mid:.3f}: {len(want)} labels; offline greedy_decode "
             f"(persistent launch, one sync): {t_off * 1e3:.2f} ms",
             f"{'chunk':>6} {'pushes':>6} {'p50 ms':>8} {'p95 ms':>8} {'stream ms':>10} {'x offline':>9}  paths  tokens"]
    for k in CHUNKS:
        def stream():
            s = model.greedy_stream(max_length=None)
            lat, paths = [], collections.Counter()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(0, T, k):
                a = time.perf_counter()
                s.push_encoded(mel[..., i:i + k])
                lat.append(time.perf_counter() - a)
                paths[s.last_path] += 1
            return time.perf_counter() - t0, lat, paths, list(s.tokens)

        stream()  # warm-up
        res = [stream() for _ in range(REPS)]
        res.sort(key=lambda r: r[0])
        total, lat, paths, toks = res[REPS // 2]
        lat_ms = np.asarray(lat) * 1e3
        same = "equal" if all(r[3] == want for r in res) else "DIFFER"
        lines.append(f"{k:6d} {len(lat):6d} {np.percentile(lat_ms, 50):8.3f} {np.percentile(lat_ms, 95):8.3f} {total * 1e3:10.2f} "
                     f"{total / t_off:9.2f}  {dict(paths)}  {same}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    out = os.path.join(ROOT, "profiles", "stream_decode_bench.txt")
    with open(out, "w") as f:
        f.write(f"# tools/bench_stream.py on {torch.cuda.get_device_name()}\n" + text)
    print("wrote", out)


if __name__ == "__main__":
    main()
