"""Find the frame seeds of tests/beam_lstm_oracle.py (SEEDS, CAPS) on the CPU: per (case, beam) the first seed of 0 .. 119, at the
shortest T of 6, 8, 10, whose float64 oracle search satisfies beam_lstm_oracle.premises — the keep / drop gap above GAP, entries of two
lengths, one of 3 or more labels.  Prints the two tables as Python source.

    python tools/find_beam_lstm_seeds.py [processes]
    python tools/find_beam_lstm_seeds.py [processes] ref     # REF_SEED: the reference's widths, T = 6, beam 4, seeds 300 .. 399
"""
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("wiring", "wiring_text", "hd36_e20", "hd256", "hd260", "l3_noln", "blank_5")
BEAMS = (2, 4, 16)
CAP_CONFIGS = (("blank_5", 16, 2, 10), ("blank_5", 16, 5, 10), ("blank_5", 4, 200, 2), ("wiring_text", 16, 5, 10), ("wiring_text", 4, 200, 2))


def find(job):
    import torch
    torch.set_num_threads(1)
    from tests import beam_lstm_oracle as bo
    name, beam, ml, m = job
    for T in (6, 8, 10):
        for seed in range(120):
            nbest, _, gap = bo.beam_oracle.beam_search(bo.Model(bo.model_of(name), bo.mel_of(name, T, seed)), beam, ml, m)
            ok = bo.premises(nbest, gap, ml)
            if ok and m < 10:  # the cap on the labels per frame must bind: another list than the uncapped search's
                ok = [y for y, _ in nbest] != [y for y, _ in bo.beam_oracle.beam_search(
                    bo.Model(bo.model_of(name), bo.mel_of(name, T, seed)), beam, ml, 10)[0]]
            if ok:
                return job, (T, seed, gap, max(len(y) for y, _ in nbest))
    return job, None


def find_ref(seed):
    import torch
    torch.set_num_threads(1)
    from tests import beam_lstm_oracle as bo
    nbest, _, gap = bo.oracle("reference_widths", bo.REF_T, seed, bo.REF_BEAM)
    return seed, gap, bo.premises(nbest, gap), max(len(y) for y, _ in nbest)


if __name__ == "__main__":
    if sys.argv[-1] == "ref":
        with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 2 else 8) as pool:
            for seed, gap, ok, longest in pool.imap(find_ref, range(300, 400)):
                print(f"seed {seed}: gap {gap:.1e} longest {longest} {'OK' if ok else ''}", flush=True)
        sys.exit(0)
    jobs = [(n, b, 200, 10) for n in NAMES for b in BEAMS] + list(CAP_CONFIGS)
    with multiprocessing.Pool(int(sys.argv[1]) if len(sys.argv) > 1 else 8) as pool:
        found = dict(pool.map(find, jobs, chunksize=1))
    for job in jobs:
        (name, beam, ml, m), hit = job, found[job]
        if hit is None:
            print(f"    # {job}: none of 3 x 120 seeds")
            continue
        T, seed, gap, longest = hit
        key = f'("{name}", {beam})' if (ml, m) == (200, 10) else f'("{name}", {beam}, {ml}, {m})'
        print(f"    {key}: ({T}, {seed}),  # gap {gap:.1e}, longest entry {longest} labels")
