"""What tests/test_arena_cpu.py and tests/test_gpu_arena_inputs.py share: tests/arena_driver.cpp built with plain g++, its input lines and
the names of its output columns."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "juicer_amd", "csrc")
SIZES = ["rec_bytes_small", "rec_bytes_large", "path_rec", "tok", "item", "state_rec", "gc_words", "tot_n", "maxw", "hist_bins", "sw"]
CAPS_IN = ["free_bytes", "cached_bytes", "mem_fraction", "B", "n_arcs", "n_states", "Fc", "n_gmm", "max_n", "cap_slots", "cap_items", "cap_paths",
           "slots_hint"]
CAPS_OUT = ["status", "passes", "cap_slots", "cap_items", "cap_paths", "cap_new", "gc_threshold", "bytes"]
PIECES = ["rec", "live", "srec", "items", "newl", "dirtyl", "tot", "item_end", "paths", "paths2", "gc_idx", "gc_state", "hist"]   # (AR_*, in order)


def caps_line(i, sizes):
    return "caps " + " ".join(str(i[k]) for k in CAPS_IN) + " " + " ".join(str(sizes[k]) for k in SIZES)


def wave_line(i):
    return "wave %d %d %d %d %d %d " % (len(i["ulen"]), i["free_bytes"], i["ll_cap"], i["G"], i["fc_env"], i["tile"]) + \
        " ".join(str(x) for x in i["ustart"] + i["ulen"])


def build_driver(path, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.check_call([gxx, "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", *extra, "-I", CSRC, "-o", path,
                           os.path.join(HERE, "arena_driver.cpp")])
    return path


def run_driver(driver, lines):
    text = "%d\n" % len(lines) + "\n".join(lines) + "\n"
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines)
    return [[int(x) for x in l.split()] for l in out]
