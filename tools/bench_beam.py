"""Beam search of one synthetic utterance (T = 1000 frames, ConvPredictor E = 512, O = H = V = 1024: the fullcausal config's widths) on
the device (RNNTModel.beam_search -> rnnt_engine_beam_decode) against the plain-torch host loop of the same search on the same GPU
(RNNTModel._beam_search_host), beams 1 / 4 / 8 / 16.  Median of `--reps` timed runs after warm-ups; writes the table to --out
(default profiles/beam_decode_bench.txt).  --host-beams: the beams the (slow) host loop is timed at."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import rnnt_amd  # noqa: E402


class Enc(torch.nn.Module):
    def forward(self, x):
        return x  # (1, H, T) already

    def calc_output_lens(self, lens):
        return lens


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--beams", default="1,4,8,16")
    ap.add_argument("--host-beams", default="1,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--blank-bias", type=float, default=1.5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "beam_decode_bench.txt"))
    a = ap.parse_args()
    torch.manual_seed(0)
    T, E, H, V = a.T, 512, 1024, 1024
    model = rnnt_amd.RNNTModel(rnnt_amd.ConvPredictor(V, H, E, 0.3), Enc(), rnnt_amd.JointNetwork(-1, -1, H, V)).cuda().eval()
    with torch.no_grad():
        model.joint.joint_ln.bias[V - 1] += a.blank_bias  # blank wins most frames, as in a trained model
    mel = torch.randn(1, H, T, device="cuda")
    lens = torch.tensor([T], device="cuda")
    audio = mel.permute(0, 2, 1)
    lines = [f"beam search, one utterance: T={T}, ConvPredictor E={E} O={H}, joint H={H} V={V}, max_length=200, 10 symbols per frame, "
             f"blank bias +{a.blank_bias}; median of {a.reps} runs after warm-ups ({torch.cuda.get_device_name()})"]
    print(lines[0], flush=True)
    host_beams = {int(b) for b in a.host_beams.split(",") if b}
    for beam in (int(b) for b in a.beams.split(",")):
        dev = lambda: model.beam_search(mel, lens, beam_size=beam, max_length=200, return_nbest=True)  # noqa: E731
        dev()
        dev()
        t_dev, nbest = timed(dev, a.reps)
        line = f"beam {beam:2d}: device {t_dev * 1e3:9.2f} ms ({len(nbest[0][0])} tokens in the best entry)"
        if beam in host_beams:
            host = lambda: model._beam_search_host(audio, beam, 200, 10)  # noqa: E731
            t_host, hb = timed(host, 1)
            same = [h[0] for h in hb] == [d[0] for d in nbest]
            line += f"   host loop {t_host * 1e3:10.1f} ms   speed-up {t_host / t_dev:6.1f}x   same n-best: {same}"
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
