"""What the waves of the row-band kernel (k_tend_rows.h) WAIT on, read off its device assembly.  No GPU.

On gfx950 `vmcnt` counts vector-memory loads AND stores and retires them in order.  The new qo leaves a strip in 16-byte
write-through stores that live in inline asm (qg_store16_wt), which the compiler does not count: a wait it places behind
one of them for a load of its own - `s_waitcnt vmcnt(0)`, "for my one load" - also waits until every store in front of it
has been acknowledged.  Two such places stood on the kernel's critical path:

  * a per-row vector load of the wave-uniform yporel inside the point-wise epilogue, consumed behind the row's stores:
    four drains per strip;
  * the table loads of the transform's front half (twid, sintab) directly behind the workgroup barrier, queued behind the
    stores of the wave's last strip.

The test compiles k_tend_rows.hip to assembly with the Makefile's own flags (HIPCC, ARCH, HIPFLAGS are read from
q-gcm_amd/csrc/Makefile; a few seconds) into a temporary directory and asserts, for both instantiations (ZM = 3, 0):

Epilogue check.  Between a strip body's first write-through store and the end of that body there is no vector-memory
load and no `s_waitcnt` that carries a `vmcnt` field.

Barrier check.  No vector-memory load stands between `s_barrier` and the first `v_mul_f64` / `v_fma_f64` of phase 2.

How the regions are delimited - by control flow, not by line ranges (the compiler places cold blocks of a body, such as
a predicated store, behind the other body or behind the barrier):

  * the kernel is the text from its label to its `.Lfunc_end`; it is cut into basic blocks at every label and behind
    every branch, with the edges `s_branch` / `s_cbranch_*` / fall-through give (`s_endpgm` has none);
  * the kernel has exactly one `s_barrier`.  The write-through stores of phase 1 are the `... sc1` stores from which the
    barrier can be reached; they all lie in ONE loop - the strongly connected component of their blocks, the strip loop -
    whose header is the one block of it that is entered from outside;
  * the strip text ends in an assembler COMMENT, `; tr_strip_end 1` / `; tr_strip_end 0` (an inline asm without
    instructions): the compiler lays the two bodies out one behind the other and skips the second with a flag register
    in place of an else branch, so the edges alone lead from the wall body into the wall-free one;
  * "from a store to the end of its body" is everything reachable from the instruction behind the store along edges that
    stay inside that loop and do not enter its header, each path ending at the first end marker it meets - exactly one
    of the two markers for any store;
  * a store that no other store reaches is the first of its body: there must be exactly two, one per marker, of 3 B = 12
    stores each, and what lies behind the first store covers the whole of the body's epilogue;
  * the barrier check walks every path from the instruction behind `s_barrier` and ends a path at its first `v_mul_f64`
    / `v_fma_f64` or at `s_endpgm`.

On the source of the commit before this test the epilogue check fails at `global_load_dwordx2 v[..], v11, s[..]
offset:-8` + `s_waitcnt vmcnt(0)` (and at the vmcnt(12) / vmcnt(11) waits between the stores of a body's first row) in
every body, the barrier check at the first `global_load_dwordx4` of dst64_front."""
import os
import re
import shlex
import subprocess

import pytest

KERNELS = {zm: "_Z11k_tend_rowsILi3ELi4ELi%dEEvPKdPK15HIP_vector_typeIdLj2EES1_iiii12QgTendParams" % zm for zm in (3, 0)}
VMEM_LOAD = re.compile(r"^(global|flat|scratch|buffer|tbuffer)_(load|atomic)|^image_")
WT_STORE = re.compile(r"^global_store_dwordx4\b.*\bsc1\b")
BRANCH = re.compile(r"^(s_branch|s_cbranch_\w+)\s+(\S+)")
NO_FALLTHROUGH = ("s_branch", "s_endpgm")
FP64_MUL = re.compile(r"^v_(mul|fma)_f64\b")
MARKER = re.compile(r"^; tr_strip_end ([01])\b")  # k_tend_rows_strip.inc: the end of the body with TR_WALLS 1 / 0


def makefile_command(csrc):
    """[hipcc, flags ...] as the Makefile's `asm` target runs it: the defaults of HIPCC, ARCH and HIPFLAGS."""
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    var = {}
    for name in ("HIPCC", "ARCH", "HIPFLAGS"):
        hit = re.findall(r"^%s\s*\?=\s*(.*)$" % name, text, flags=re.M)
        assert len(hit) == 1, (name, hit)
        var[name] = hit[0].strip()
    flags = var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"])
    assert "$" not in flags, flags
    return [os.environ.get("HIPCC", var["HIPCC"])] + shlex.split(flags)


@pytest.fixture(scope="module")
def band_asm(repo_root, tmp_path_factory):
    csrc = os.path.join(repo_root, "q-gcm_amd", "csrc")
    out = str(tmp_path_factory.mktemp("band_asm") / "k_tend_rows.s")
    cmd = makefile_command(csrc) + ["--cuda-device-only", "-S", "-o", out, "k_tend_rows.hip"]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return open(out).read()


class Kernel:
    """Basic blocks and edges of one kernel of an assembly listing."""

    def __init__(self, asm, name):
        lines = asm.split("\n")
        start = [i for i, l in enumerate(lines) if l.startswith(name + ":")]
        assert len(start) == 1, (name, start)
        end = next(i for i in range(start[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
        self.ins = []      # (line number in the listing, instruction text)
        label_at = {}      # label -> index of the first instruction behind it
        for i in range(start[0] + 1, end):
            l = lines[i].split(";")[0].strip() if not lines[i].lstrip().startswith(";") else ""
            m = MARKER.match(lines[i].strip())
            if m:  # (kept as a pseudo-instruction)
                l = "tr_strip_end " + m.group(1)
            if not l or l.startswith("."):
                m = re.match(r"^(\.LBB\w+):", l)
                if m:
                    label_at[m.group(1)] = len(self.ins)
                continue
            self.ins.append((i + 1, l))
        n = len(self.ins)
        assert n > 1000 and not any(re.match(r"^s_(setpc|swappc|call)", t) for _, t in self.ins), name
        leaders = {0} | set(label_at.values())
        for k, (_, t) in enumerate(self.ins):
            if BRANCH.match(t) or t.startswith("s_endpgm"):
                leaders.add(k + 1)
        leaders = sorted(x for x in leaders if x < n)
        self.block_of = [0] * n
        self.blocks = []   # (first, last + 1)
        for b, first in enumerate(leaders):
            last = leaders[b + 1] if b + 1 < len(leaders) else n
            self.blocks.append((first, last))
            for k in range(first, last):
                self.block_of[k] = b
        self.succ = []
        for b, (first, last) in enumerate(self.blocks):
            t = self.ins[last - 1][1]
            s = set()
            m = BRANCH.match(t)
            if m:
                assert m.group(2) in label_at, t
                s.add(self.block_of[label_at[m.group(2)]])
            if not t.startswith(NO_FALLTHROUGH) and last < n:
                s.add(b + 1)
            self.succ.append(sorted(s))

    def reach(self, blocks, allowed=None, stop=()):
        """Blocks reachable from the SUCCESSORS of `blocks` (along edges inside `allowed`, never entering `stop`)."""
        seen, todo = set(), list(blocks)
        while todo:
            for s in self.succ[todo.pop()]:
                if s not in seen and s not in stop and (allowed is None or s in allowed):
                    seen.add(s)
                    todo.append(s)
        return seen

    def find(self, rx):
        return [k for k, (_, t) in enumerate(self.ins) if rx.match(t)]

    def where(self, k):
        return "line %d: %s" % self.ins[k]


def strip_loop(K):
    """(stores of phase 1, blocks of the strip loop, its header block)."""
    bar = K.find(re.compile(r"^s_barrier\b"))
    assert len(bar) == 1, [K.where(k) for k in bar]
    bar_block = K.block_of[bar[0]]
    stores = [k for k in K.find(WT_STORE)
              if bar_block in K.reach([K.block_of[k]]) or (K.block_of[k] == bar_block and k < bar[0])]
    assert stores, "no write-through store in front of the barrier"
    blocks = {K.block_of[k] for k in stores}
    first = min(blocks)
    down = K.reach([first]) | {first}
    loop = {b for b in down if first in K.reach([b])} | ({first} if first in K.reach([first]) else set())
    assert blocks <= loop, "the write-through stores of phase 1 do not all lie in one loop"
    assert bar_block not in loop
    pred_outside = {s for b in range(len(K.blocks)) if b not in loop for s in K.succ[b] if s in loop}
    assert len(pred_outside) == 1, ("the strip loop has one header", sorted(pred_outside))
    return stores, loop, pred_outside.pop()


def behind(K, k, loop, header):
    """(instruction indices from behind instruction k to the end of its strip body, the end markers met) - see the
    module docstring."""
    out, ends, seen = [], set(), set()
    todo = [(K.block_of[k], k + 1)]
    while todo:
        b, k0 = todo.pop()
        for i in range(k0, K.blocks[b][1]):
            if K.ins[i][1].startswith("tr_strip_end"):
                ends.add(K.ins[i][1])
                break
            out.append(i)
        else:
            for s in K.succ[b]:
                if s in loop and s != header and s not in seen:
                    # (reaching k's own block again would be a loop inside the strip: there is none)
                    assert s != K.block_of[k], K.where(k)
                    seen.add(s)
                    todo.append((s, K.blocks[s][0]))
    return out, ends


@pytest.mark.parametrize("zm", [3, 0])
def test_no_vector_memory_wait_behind_a_strips_first_store(band_asm, zm):
    K = Kernel(band_asm, KERNELS[zm])
    stores, loop, header = strip_loop(K)
    tails, ends = {}, {}
    for k in stores:
        tails[k], ends[k] = behind(K, k, loop, header)
        assert len(ends[k]) == 1, ("a store lies in ONE body and that body's end marker is behind it", K.where(k), ends[k])
    firsts = [k for k in stores if not any(k in tails[o] for o in stores if o != k)]
    sizes = sorted(1 + sum(o in tails[k] for o in stores) for k in firsts)
    print(zm, "stores", len(stores), "bodies", [(K.where(k), ends[k]) for k in firsts], sizes)
    assert len(firsts) == 2 and sizes == [12, 12], ("two strip bodies of 3 layers x 4 rows of stores", sizes)
    assert set.union(*(ends[k] for k in firsts)) == {"tr_strip_end 0", "tr_strip_end 1"}
    bad = []
    for k in firsts:
        for i in tails[k]:
            t = K.ins[i][1]
            if VMEM_LOAD.match(t) or (t.startswith("s_waitcnt") and ("vmcnt" in t or re.match(r"^s_waitcnt\s+(0x|\d)", t))):
                bad.append("behind the store at %s -> %s" % (K.where(k), K.where(i)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("zm", [3, 0])
def test_no_vector_memory_load_between_the_barrier_and_the_transform(band_asm, zm):
    K = Kernel(band_asm, KERNELS[zm])
    bar = K.find(re.compile(r"^s_barrier\b"))
    assert len(bar) == 1
    bad, muls, seen = [], [], set()
    todo = [(K.block_of[bar[0]], bar[0] + 1)]
    while todo:
        b, k0 = todo.pop()
        for i in range(k0, K.blocks[b][1]):
            t = K.ins[i][1]
            if VMEM_LOAD.match(t):
                bad.append(K.where(i))
            if FP64_MUL.match(t):
                muls.append(i)
                break
        else:
            for s in K.succ[b]:
                if s not in seen:
                    seen.add(s)
                    todo.append((s, K.blocks[s][0]))
    print(zm, "barrier at", K.where(bar[0]), "first fp64 products at", [K.where(i) for i in sorted(muls)])
    assert muls, "phase 2 has fp64 products"
    assert not bad, "\n".join(bad)
