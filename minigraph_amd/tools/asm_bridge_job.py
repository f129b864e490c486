"""profiles/asm_bridge_wgx.txt, the job rows: -cx asm over mgsim -G 200000000 -n 10 -l 20000000, MGA_ASM_DEV_BRIDGE unset and =1, alternated, three runs each; one child process per run"""
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
         "t = time.time()\nmga.map_files(sys.argv[1], [sys.argv[2]], sys.argv[3], preset='asm', cigar=True, n_threads=16, verbose=0)\n"
         "print('JOB', time.time() - t, *mga.asm_bridge_stats().values())\n") % ROOT

def say(*a):
    print(*a, flush=True)

d = tempfile.mkdtemp()
t = time.time()
subprocess.check_call([mga.MGSIM, "-p", os.path.join(d, "t"), "-G", "200000000", "-H", "3", "-n", "10", "-l", "20000000", "-e", "0.004", "-s", "5"], stderr=subprocess.DEVNULL, timeout=300)
say("mgsim", round(time.time() - t, 1), "s")
graph, reads = os.path.join(d, "t.gfa"), os.path.join(d, "t.reads.fa")
ref = None
for rep in range(3):
    for mode in (None, "1"):
        env = {k: v for k, v in os.environ.items() if k != "MGA_ASM_DEV_BRIDGE"}
        if mode:
            env["MGA_ASM_DEV_BRIDGE"] = mode
        o = os.path.join(d, "o.gaf")
        r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
        t = time.time()
        p = subprocess.run([sys.executable, "-c", CHILD, graph, reads, o], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=170)
        wall = time.time() - t
        r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
        if p.returncode != 0:   # nothing more on the GPU after a failed run
            say("FAILED", mode, p.returncode, p.stderr.decode()[-1500:])
            sys.exit(1)
        gaf = open(o, "rb").read()
        ref = ref if ref is not None else gaf
        job = [l for l in p.stdout.decode().splitlines() if l.startswith("JOB")][0].split()[1:]
        say("rep", rep, "MGA_ASM_DEV_BRIDGE", mode or "unset", "process wall %.2f s" % wall, "map_files %.2f s" % float(job[0]),
            "host CPU-s %.2f" % (r1.ru_utime + r1.ru_stime - r0.ru_utime - r0.ru_stime), "wide/back/host", job[1:], "gaf bytes", len(gaf), "same as first", gaf == ref)
