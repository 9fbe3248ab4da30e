"""CPU tests of the layout of csrc/: the build's hand-kept header list against the files that exist and the includes that are
written, and the include rule of the rollout kernels' headers (one header per concern; a translation unit
sees a kernel family's header only if it launches that family).  Includes are followed textually; nothing is compiled."""
import os
import re

from ccv_mppi_path_tracker_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
# the kernel headers, one per family, and the units that launch each family (every other source sees none of them)
FAMILY_HEADERS = {"plain": "mppi_rollout_plain.h", "pc": "mppi_rollout_pc.h", "r3": "mppi_rollout_r3.h", "r4": "mppi_rollout_r4.h",
                  "solo": "mppi_rollout_solo.h"}
LAUNCHES = {"k_plain.hip": {"plain"}, "k_pc.hip": {"pc"}, "k_pc_fb.hip": {"pc"}, "k_r3.hip": {"r3"}, "k_r4.hip": {"r4"},
            "k_r4_fb.hip": {"r4"}, "k_solo.hip": {"solo"}, "k_solo_fb.hip": {"solo"}}
BATCH_FAMILIES = {"plain", "r4", "solo"}   # k_batch*.hip (k_batch_form.h)


def _norm(path):
    return os.path.normpath(os.path.join(build.CSRC, path))


def _includes(path):
    """the quoted includes of one file, as normalised absolute paths"""
    with open(path) as f:
        return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in INCLUDE.findall(f.read())]


def _reachable(path):
    """every file the quoted includes of `path` reach, transitively"""
    seen, todo = set(), [path]
    while todo:
        for inc in _includes(todo.pop()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    return seen


def test_every_header_is_a_build_dependency():
    deps = {_norm(d) for d in build.DEPS}
    missing = [d for d in deps if not os.path.exists(d)]
    assert not missing, missing
    headers = {_norm(h) for h in build.HEADERS}
    on_disk = {os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith(".h")}
    assert on_disk <= headers, sorted(os.path.basename(h) for h in on_disk - headers)
    # every include that is written resolves to a file the staleness check looks at
    for src in sorted(deps):
        for inc in _includes(src):
            assert inc in deps, "%s includes %s, which is not in build.DEPS" % (os.path.relpath(src, build.CSRC), os.path.relpath(inc, build.CSRC))


def test_a_unit_sees_only_the_kernel_headers_of_the_families_it_launches():
    family_of = {_norm(h): fam for fam, h in FAMILY_HEADERS.items()}
    for h in family_of:
        assert os.path.exists(h), h
    batch_units = [u for u in build.KERNEL_UNITS if u.startswith("k_batch")]
    assert len(batch_units) == 9
    for unit in build.SOURCES:
        allowed = BATCH_FAMILIES if unit in batch_units else LAUNCHES.get(unit, set())
        seen = {family_of[p] for p in _reachable(_norm(unit)) if p in family_of}
        assert seen == allowed, "%s reaches the kernel headers of %s, launches %s" % (unit, sorted(seen), sorted(allowed))
    # the rule as the four-wave, one-wave and batch units are held to it: neither the two-wave nor the three-wave kernel is parsed
    for unit in ["k_r4.hip", "k_r4_fb.hip", "k_solo.hip", "k_solo_fb.hip"] + batch_units:
        reach = {os.path.basename(p) for p in _reachable(_norm(unit))}
        assert not reach & {"mppi_rollout_pc.h", "mppi_rollout_r3.h"}, (unit, sorted(reach))
    # the kernel headers build on the building blocks, not on each other
    for h in family_of:
        assert not {p for p in _reachable(h) if p in family_of}, os.path.basename(h)


def _reaching(header):
    """the sources (build.SOURCES) that reach csrc/<header>"""
    return {unit for unit in build.SOURCES if _norm(header) in _reachable(_norm(unit))}


def test_the_inflation_tile_body_is_seen_by_the_two_units_that_run_it():
    assert os.path.exists(_norm("mppi_costmap_device.h"))
    assert _reaching("mppi_costmap_device.h") == {"k_costmap.hip", "k_costmap_roll.hip"}


def test_the_configuration_unit_sees_no_costmap_header():
    assert "capi_batch_maps.hip" in build.CAPI_UNITS
    reach = {os.path.basename(p) for p in _reachable(_norm("capi_batch_config.hip"))}
    assert not {h for h in reach if h.startswith("mppi_costmap")}, sorted(reach)
    assert {"mppi_costmap.h", "mppi_costmap_roll.h", "mppi_costmap_scan.h"} <= {os.path.basename(p) for p in _reachable(_norm("capi_batch_maps.hip"))}


def test_the_row_pass_of_the_inflation_stands_in_one_file():
    # (kNone is the row pass's "no occupied cell within R": where it is defined, the pass is written)
    holders = []
    for name in sorted(os.listdir(build.CSRC)):
        path = os.path.join(build.CSRC, name)
        if os.path.isfile(path):
            with open(path) as f:
                holders += [name] * len(re.findall(r"^\s*constexpr\s+int\s+kNone\b", f.read(), re.M))
    assert holders == ["mppi_costmap_device.h"], holders
