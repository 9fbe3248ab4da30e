"""CPU tests of who owns device memory, pinned memory and events on the host side of the C ABI: the text of csrc/ is read, nothing
is compiled.  The allocation and free calls of the HIP runtime stand in csrc/capi_owned.h, whose holders give back what they hold
when they go, and in csrc/capi_exchange.hip, whose box is opened and closed through IPC handles; a handle's part (capi_internal.h)
has no release() to forget a pointer in.  This is the check that no owner was missed, down to the allocations too small for a
reading of the device's free memory to see (tests/test_gpu_batch_lifecycle.py): the [B] tables of the fleet term, the plan's result
rows, the sensing read-back."""
import os
import re

from ccv_mppi_path_tracker_amd import build

OWNERS = {"capi_owned.h", "capi_exchange.hip"}
RAW = ("hipMalloc(", "hipHostMalloc(", "hipFree(", "hipHostFree(", "hipEventCreate", "hipEventDestroy", "free_device")


def host_sources():
    """{name relative to csrc/: text} of csrc/*.hip, csrc/*.h and csrc/host/*"""
    out = {}
    for name in sorted(os.listdir(build.CSRC)):
        if name.endswith((".hip", ".h")):
            out[name] = os.path.join(build.CSRC, name)
    host = os.path.join(build.CSRC, "host")
    for name in sorted(os.listdir(host)):
        if os.path.isfile(os.path.join(host, name)):
            out[os.path.join("host", name)] = os.path.join(host, name)
    texts = {}
    for name, path in out.items():
        with open(path) as f:
            texts[name] = f.read()
    return texts


def test_the_sources_are_all_there():
    texts = host_sources()
    assert OWNERS <= set(texts) and "capi_internal.h" in texts and len(texts) > 60, sorted(texts)
    for word in RAW[:6]:   # (what the search below looks for is written where it is allowed)
        assert any(word in texts[o] for o in OWNERS), word


def test_raw_allocation_calls_stand_in_the_owners_alone():
    found = [(name, word) for name, text in host_sources().items() if name not in OWNERS for word in RAW if word in text]
    assert not found, found


def test_no_part_of_a_handle_has_a_release():
    text = host_sources()["capi_internal.h"]
    assert "struct ccv_mppi_batch" in text and "struct Costmap" in text
    assert not re.findall(r"\brelease\s*\(\s*\)\s*\{", text), "a part defines release()"
    assert not re.findall(r"\bvoid\s+release\s*\(", text), "a part declares release()"
