"""Build the reference itself into oracle/_ref/ — TEST INFRASTRUCTURE ONLY.

The reference (MacSpain/cpu-renderer: projekt.cpp, projekt.h) is not part of
this repository and none of its text is.  This recipe addresses it by path,
checks that it is the revision the fixtures were drawn from (SHA-256), writes
a lane-rewritten copy of its source under oracle/_ref/ (never into the tree)
and compiles oracle/ref/ref_driver.cpp around it with oracle/ref/prelude.h
force-included.

  python oracle/ref/build_ref.py [--sanitize]

PRK_REFERENCE_DIR names the reference's directory (default /root/reference).
Where it does not exist nothing is built: tests/golden/ref/ holds what the
reference drew, and only the live cross-check of tests/test_ref_parity.py
needs the driver.
"""
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")

HASHES = {
    "projekt.cpp": "f5b2d180aabf9af909a781d39cb36690bd902e9ba956ea13c823c23b294b0e76",
    "projekt.h": "7fa062006e8d07a90050638fc8ab695177c660a3ac5d55914e6c4e5aaf7fd08c",
}
CXX = "g++"
FLAGS = ["-std=c++17", "-O2", "-mavx2", "-mno-fma", "-ffp-contract=off"]
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]

# Member access to a lane of a vector value (`V.m256i_u32[k]` and its kin, a
# spelling one compiler family has) becomes LANE_<bits>_<type>(V, k), which
# prelude.h defines.  Generic: it quotes nothing of the text it is run over.
LANE = re.compile(r"\b([A-Za-z_][A-Za-z0-9_.]*)\.m(256|128)i?_(u32|i32|f32)\[([0-9])\]")
LANE_SITES = 494

# What the absent platform and math headers would decide, decided by prelude.h.
PINS = [
    "RoundR32ToS32(x) = (s32)roundf(x), RoundR32ToU32(x) = (u32)roundf(x): halves away from zero",
    "Normalize(a) = (1/sqrtf(Inner(a,a)))*a",
    "Inner(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z",
    "Clamp01(x) = x<0 ? 0 : (x>1 ? 1 : x), per component",
    "Sin/Cos = sinf/cosf of the host libm; Pi32 = 3.14159265359f",
    "vector arithmetic is component-wise, one IEEE single operation each, nothing fused",
    "Platform.AddEntry runs the entry at once on the calling thread (synchronous queue)",
    "_InterlockedCompareExchange8 = __sync_val_compare_and_swap, _WriteBarrier = compiler barrier",
    "Assert throws; an object whose FillEdgeTable asserts in its sort (no visible edge) is not drawn",
    "clear values: colour 0xFF000000, z -FLT_MAX; ZMask zeroed; fresh EdgeMemory zeroed",
    "light_data holds 8 lights; textures carry one zeroed guard row (Height+1 rows)",
]
# Edits to the reference's text beyond the lane rewrite.  The default driver
# (ref_driver) has none.  The texture lives inside an arena of the driver's own
# that spans every signed 32-bit byte offset, so the reads of masked-out lanes
# and of u = v = 1 land in memory the driver owns (SURVEY's P2 / P4 clamps are
# not needed); every scene is drawn with two fills of the arena's near part
# and a pixel that differs is reported (and refused by
# tools/make_ref_golden.py).  An object with no visible edge fails the Assert
# of the reference's sort and is not drawn (P1 is not needed).
#
# P3: when the first pair of the active edge list swaps, the
# reference leaves its list head and tail behind.  With two edges listed its
# next row walks off the list's end (a null dereference) unless the swap was
# on the object's last row, which most soups do somewhere; with more edges
# listed it survives, and the edge that moved to the front is no longer in the
# list.  A second driver (ref_driver_p3) is built with the head and tail
# carried along at the swap, in all four copies of the walk: that is the
# behaviour this project restates (oracle, pyref, CPU baseline, kernels).  Each
# site is addressed by line: text of our own is appended to the line that
# closes the swap's inner block (which must consist of one closing brace).
# tools/make_ref_golden.py draws every case with both drivers and records per
# case what the unpatched one did (same frame, crash, or a different frame).
PATCHES = {
    "P3": dict(lines=[569, 3326, 3573, 3838], expect=r"^\s*\}\s*$",
               append=" else ListHead = NextEdgeInList;"
                      " if(ListTail == NextEdgeInList) ListTail = CurrentEdgeInList;",
               what="first-pair swap of the active edge list also updates the list's head and tail; the unpatched "
                    "walk then runs off its list (two edges listed) or goes on without the edge that moved to the "
                    "front (more edges listed)"),
}


class ReferenceMismatch(RuntimeError):
    pass


def reference_dir():
    return os.environ.get("PRK_REFERENCE_DIR", "/root/reference")


def available():
    d = reference_dir()
    return all(os.path.isfile(os.path.join(d, n)) for n in HASHES)


def check_hashes():
    d = reference_dir()
    for name, want in HASHES.items():
        with open(os.path.join(d, name), "rb") as f:
            got = hashlib.sha256(f.read()).hexdigest()
        if got != want:
            raise ReferenceMismatch(
                "%s is not the revision this recipe was written for (SHA-256 %s, recorded %s): "
                "line numbers, the lane count and the fixtures under tests/golden/ref/ belong to the recorded one"
                % (os.path.join(d, name), got, want))


def driver_path(sanitize=False, patches=()):
    return os.path.join(OUT, "ref_driver" + "".join("_" + p.lower() for p in patches) + ("_san" if sanitize else ""))


def apply_patch(text, name):
    p = PATCHES[name]
    lines = text.split("\n")
    for no in p["lines"]:
        line = lines[no - 1].rstrip("\r")
        if not re.match(p["expect"], line):
            raise ReferenceMismatch("patch %s: line %d is not what the recipe expects" % (name, no))
        lines[no - 1] = line + p["append"] + lines[no - 1][len(line):]
    return "\n".join(lines)


def compiler_version():
    return subprocess.run([CXX, "--version"], check=True, capture_output=True, text=True).stdout.splitlines()[0]


def build(sanitize=False, quiet=False, patches=()):
    """Compile the driver (with the named PATCHES applied to the rewritten
    copy); returns its path, or None when there is no reference (one line says
    so)."""
    if not available():
        if not quiet:
            print("oracle/ref: no reference at %s, driver not built (fixtures under tests/golden/ref/ stand in)"
                  % reference_dir())
        return None
    check_hashes()
    os.makedirs(OUT, exist_ok=True)
    d = reference_dir()
    with open(os.path.join(d, "projekt.cpp"), "r", encoding="utf-8", errors="surrogateescape", newline="") as f:
        text = f.read()
    text, sites = LANE.subn(r"LANE_\2_\3(\1,\4)", text)
    if sites != LANE_SITES:
        raise ReferenceMismatch("lane rewrite touched %d sites, expected %d" % (sites, LANE_SITES))
    for name in patches:
        text = apply_patch(text, name)
    rewritten = os.path.join(OUT, "projekt_lanes%s.cpp" % "".join("_" + p.lower() for p in patches))
    with open(rewritten, "w", encoding="utf-8", errors="surrogateescape", newline="") as f:
        f.write(text)
    exe = driver_path(sanitize, patches)
    cmd = ([CXX] + FLAGS + (SANITIZE if sanitize else []) +
           ["-w", "-include", os.path.join(HERE, "prelude.h"),
            '-DREF_HEADER="%s"' % os.path.join(d, "projekt.h"), '-DREF_SOURCE="%s"' % rewritten,
            os.path.join(HERE, "ref_driver.cpp"), "-o", exe])
    subprocess.run(cmd, check=True)
    return exe


def build_all(sanitize=False, quiet=False):
    """Both drivers: unpatched and P3."""
    return [build(sanitize, quiet, ()), build(sanitize, True, ("P3",))]


if __name__ == "__main__":
    for p in build_all(sanitize="--sanitize" in sys.argv[1:]):
        if p:
            print(p)
