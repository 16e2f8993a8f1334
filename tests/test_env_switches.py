"""The environment variables the library reads are the ones INTEGRATION.md documents, and the switches of the finished A/B
experiments (environment variables and compile-time -D hooks) are gone from everything that ships or measures."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gaussiansplatting.jl_amd")

RETIRED = (
    "GSR_SORT_TIERS_NETWORK", "GSR_TILE_ORDER", "GSR_NO_BG0", "GSR_NO_FUSED_FWD", "GSR_SPEC_TIER_SORTS", "GSR_WALK_PRIO",
    "GSR_BWD_COLOR_ONLY", "GSR_TIERS_BESIDE_MAX", "GSR_BWD_SPLIT_TILES", "GSR_AGG_MAX_BANDS",  # environment variables
    "GSR_PRE_NO_BINNING", "GSR_BWD_MINWAVES", "GSR_PGB_MINWAVES",                             # -D hooks
)


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def test_the_library_reads_exactly_the_documented_variables():
    sources = [p for ext in ("cpp", "hip", "h") for p in glob.glob(os.path.join(PKG, "csrc", "*." + ext))]
    assert len(sources) >= 10, sources
    read_by_library = {name for p in sources for name in re.findall(r'getenv\(\s*"(GSR_\w+)"\s*\)', read(p))}
    section = read(os.path.join(ROOT, "INTEGRATION.md")).split("## Environment variables read by the library", 1)[1]
    section = section.split("\n## ", 1)[0]
    documented = set(re.findall(r"^\| `(GSR_\w+)", section, re.M))
    assert documented, "no table of variables in INTEGRATION.md"
    assert read_by_library == documented, (sorted(read_by_library - documented), sorted(documented - read_by_library))


def test_no_retired_switch_is_left():
    files = [os.path.join(ROOT, "bench.py")]
    files += glob.glob(os.path.join(ROOT, "tools", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.sh"))
    for top in (PKG, os.path.join(ROOT, "include")):
        for d, dirs, names in os.walk(top):
            dirs[:] = [x for x in dirs if x not in ("build", "__pycache__")]
            files += [os.path.join(d, n) for n in names if not n.endswith((".so", ".o", ".pyc"))]
    assert len(files) > 40, len(files)
    pattern = re.compile(r"\b(" + "|".join(RETIRED) + r")\b")
    left = sorted({(os.path.relpath(p, ROOT), m) for p in files for m in pattern.findall(read(p))})
    assert not left, left
