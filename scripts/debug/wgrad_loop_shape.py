"""Shape of a weight-gradient kernel's MFMA loop, read from the device assembly (no GPU).

  hipcc <the flags of csrc/build.py> -S --cuda-device-only mi-seg_amd/csrc/conv3d.hip -o conv3d.s
  python scripts/debug/wgrad_loop_shape.py conv3d.s [--kernel SUBSTRING ...] [--string N]

Per matching kernel: the resource line (VGPRs / AGPRs / scratch), the instruction counts of the longest run of code that holds MFMAs,
and that run as one letter per instruction:

  M  v_mfma                       D  ds_read (the transposed LDS fragment reads)      S  ds_write
  W  s_waitcnt with an lgkmcnt    w  s_waitcnt on vmcnt alone                          G  global / buffer / scratch load or store
  v  any other vector instruction s  any other scalar instruction                      |  a label or branch (basic-block edge)

and what the prefetch is judged by: for every MFMA, how many MFMAs lie between it and the closest LDS wait in front of it whose counter
lets fewer reads stay in flight than were issued since the wait before ("exposed" = a wait with at most `--near` MFMAs in front of it that
follows reads issued inside the same gap); `read -> wait -> single MFMA` triples are counted as such."""
import argparse
import re
import sys


def kernels(path):
    name, body, out = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        body.append(line.rstrip("\n"))
    return out


def resources(path):
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(path).read(), re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        res[m.group(1)] = d
    return res


def lgkm(op):
    """the lgkmcnt of an s_waitcnt operand string, None when it does not wait on it"""
    m = re.search(r"lgkmcnt\((\d+)\)", op)
    if m:
        return int(m.group(1))
    m = re.match(r"\s*(0x[0-9a-fA-F]+|\d+)\s*$", op)
    if m:
        return (int(m.group(1), 0) >> 8) & 0xF
    return None


def classify(body):
    s = []
    for line in body:
        t = line.strip()
        if not t or t.startswith((";", ".")) and not t.startswith(".LBB"):
            continue
        if t.startswith(".LBB"):
            s.append(("|", None))
            continue
        op, _, rest = t.partition(" ")
        if op.startswith("v_mfma"):
            s.append(("M", None))
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            s.append(("D", None))
        elif op.startswith("ds_"):
            s.append(("S", None))
        elif op == "s_waitcnt":
            n = lgkm(rest.split(";")[0])
            s.append(("W", n) if n is not None else ("w", None))
        elif op.startswith(("global_", "buffer_", "scratch_", "flat_")):
            s.append(("G", None))
        elif op.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier")):
            s.append(("|", None))
        elif op.startswith("v_"):
            s.append(("v", None))
        elif op.startswith("s_"):
            s.append(("s", None))
    return s


def longest_mfma_run(seq):
    """the basic block (run between edges) with the most MFMAs"""
    best, cur = [], []
    for it in seq + [("|", None)]:
        if it[0] == "|":
            if sum(1 for c, _ in cur if c == "M") > sum(1 for c, _ in best if c == "M"):
                best = cur
            cur = []
        else:
            cur.append(it)
    return best


def judge(run, near):
    counts = {c: sum(1 for k, _ in run if k == c) for c in "MDSWwGvs"}
    triples = exposed = 0
    letters = "".join(c for c, _ in run)
    triples = len(re.findall(r"D[vs]*W[vs]*M(?=[vs]*D)", letters))
    # an LDS wait is exposed when reads were issued since the last MFMA burst of more than `near` MFMAs and the wait drains them
    pending_since, mf = 0, 0
    for c, n in run:
        if c == "D":
            pending_since += 1
            if mf > near:
                mf = 0
        elif c == "M":
            mf += 1
        elif c == "W":
            if pending_since and n < pending_since and mf <= near:
                exposed += 1
            pending_since = min(pending_since, n)
            mf = 0
    return counts, triples, exposed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", action="append", default=None, help="substring of the mangled name (default: the bf16 weight-gradient kernels)")
    ap.add_argument("--string", type=int, default=0, help="print this many letters of the run, from its first MFMA (0: none)")
    ap.add_argument("--skip", type=int, default=0, help="letters to skip behind the first MFMA before printing")
    ap.add_argument("--near", type=int, default=2, help="a wait with at most this many MFMAs since the reads it drains counts as exposed")
    a = ap.parse_args()
    want = a.kernel or ["conv3_wgrad_kernelIDF16b", "conv3_wgrad_group_kernelIDF16b"]
    ks, res = kernels(a.asm), resources(a.asm)
    for name, body in ks.items():
        if not any(w in name for w in want):
            continue
        r = res.get(name, {})
        run = longest_mfma_run(classify(body))
        counts, triples, exposed = judge(run, a.near)
        print(name)
        print(f"  next_free_vgpr {r.get('next_free_vgpr')} accum_offset {r.get('accum_offset')} private_segment_fixed_size {r.get('private_segment_fixed_size')}")
        print("  block: " + " ".join(f"{k}={v}" for k, v in counts.items()) + f"  read->wait->single-MFMA triples={triples}  exposed LDS waits={exposed}")
        if a.string:
            letters = "".join(c + (str(n) if c == "W" else "") for c, n in run)
            first = letters.find("M")
            print("  " + letters[first + a.skip:first + a.skip + a.string])
    return 0


if __name__ == "__main__":
    sys.exit(main())
