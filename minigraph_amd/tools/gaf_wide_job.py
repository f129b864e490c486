"""profiles/gaf_wide.txt, the job rows: -cx asm over mgsim -G 200000000 -n 10 -l 20000000, GAF to a file; a build of the parent commit (argv[1]: its libminigraph_amd.so) against
this one with MGA_DEV_GAF_WIDE=1, alternated, three runs each, one child process per run; then one more run of this build with the per-kernel event timing on, for the
isolated time of the wide kernel's two passes"""
import os
import resource
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import minigraph_amd as mga

CHILD = ("import sys, time; sys.path.insert(0, %r)\nimport minigraph_amd as mga\n"
         "prof = len(sys.argv) > 4\nmga.prof_enable(prof)\n"
         "t = time.time()\nmga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset='asm', cigar=True, n_threads=16, verbose=0)\nt = time.time() - t\n"
         "st = list(mga.gaf_wide_stats().values()) if hasattr(mga.load(), 'mga_gaf_wide_stats') else ['-', '-']\n"
         "print('JOB', t, *st)\n"
         "if prof: print('PROF', *['%%s=%%.3fms/%%d' %% (k, v[0], v[1]) for k, v in mga.prof_get().items() if k in ('k_gaf', 'k_gaf_wide', 'k_text')])\n") % ROOT


def say(*a):
    print(*a, flush=True)


def run(graph, reads, out, env_add, prof=False):
    env = {k: v for k, v in os.environ.items() if k not in ("MGA_DEV_GAF_WIDE", "MGA_LIB")}
    env.update(env_add)
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t = time.time()
    p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, out] + (["prof"] if prof else []), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=170)
    wall = time.time() - t
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    if p.returncode != 0:   # nothing more on the GPU after a failed run
        say("FAILED", env_add, p.returncode, p.stderr.decode()[-1500:])
        sys.exit(1)
    lines = p.stdout.decode().splitlines()
    job = [l for l in lines if l.startswith("JOB")][0].split()[1:]
    return wall, float(job[0]), r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime, job[1:], [l for l in lines if l.startswith("PROF")]


parent = os.path.abspath(sys.argv[1])
d = tempfile.mkdtemp()
t = time.time()
subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "200000000", "-H", "3", "-n", "10", "-l", "20000000", "-e", "0.004", "-s", "5"], stderr=subprocess.DEVNULL, timeout=300)
say("mgsim", round(time.time() - t, 1), "s")
graph, reads, o = os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa"), os.path.join(d, "o.gaf")
ref = None
for rep in range(3):
    for what, env in (("parent", {"MGA_LIB": parent}), ("MGA_DEV_GAF_WIDE=1", {"MGA_DEV_GAF_WIDE": "1"})):
        wall, t_map, cpu, st, _ = run(graph, reads, o, env)
        gaf = open(o, "rb").read()
        ref = ref if ref is not None else gaf
        say("rep", rep, what, "process wall %.2f s" % wall, "map_files %.2f s" % t_map, "host CPU-s %.2f" % cpu, "wide lines / chunks too long", st, "gaf bytes", len(gaf),
            "same as first", gaf == ref)
_, t_map, _, st, prof = run(graph, reads, o, {"MGA_DEV_GAF_WIDE": "1"}, prof=True)
say("event timing on: map_files %.2f s" % t_map, "wide lines", st, *prof)
