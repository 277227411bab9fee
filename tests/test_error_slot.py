"""CPU: one error slot for the whole library.  libdeepmod_hip.so is linked from several host translation units (DESIGN.md "Translation
units"); fail() and the thread-local message behind dm_last_error() are defined once, in deepmod_hip.hip, and declared to the others by
csrc/host.h.  One entry point of every host unit is called with an argument it rejects before any HIP call: it returns the documented
DM_EINVAL, and dm_last_error(), which lives in the core unit, returns that call's own message - not an empty string (a unit writing to a slot
of its own) and not the message of the call before it.  The three kernel units (kern_*.hip) have no entry point of the C ABI and do not
report through the slot at all: their launch wrappers return hipError_t to the core unit."""
from deepmod_amd import _lib

# (unit, call, message)
REJECTED = [
    ("deepmod_hip.hip", lambda lib: lib.dm_device_pci_bus_id(0, None, 0), b"dm_device_pci_bus_id: buffer of >= 13 bytes"),
    ("summary.hip", lambda lib: lib.dm_bed_format_at(None, b"+", b"C", 0, None, None, None, 0, None, 0), b"dm_bed_format: bad input"),
    ("feed.hip", lambda lib: lib.dm_map_read(0, 1, None, None, 0, None, 0, 0, None, None, None, None, 0, None), b"dm_map_read: null argument"),
    ("feed.hip", lambda lib: lib.dm_rows_info(None, None, None, None, None, None, 0, None), b"null batch"),
    ("offline.hip", lambda lib: lib.dm_xy_rows_host(None, None, None, None, 0, 0, None, 0, None, None, None, None, 0), b"dm_xy_rows_host: null array"),
]


def test_every_host_unit_reports_through_the_one_error_slot(hip_lib):
    import __graft_entry__ as ge
    assert {u for u, _, _ in REJECTED} == {u for u in ge.UNITS if not u.startswith("kern_")}
    for unit, call, message in REJECTED + REJECTED[::-1]:          # every message replaces another unit's, in both directions
        assert call(hip_lib) == _lib.DM_EINVAL, unit
        assert hip_lib.dm_last_error() == message, unit
