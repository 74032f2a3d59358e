"""The device DEFLATE coder (csrc/bam_deflate_kernels.hpp plan_match_kernel / emit_match_kernel) on the payloads of
deflate_limit_cases.py, byte for byte against the host twin: tokens that reach a third staging word (`wide`, `widest`: up to
48 bits), rounds whose store loop needs its second pass (`wide`: more than 64 words), and the Kraft repair on the ranked
286-symbol and 30-symbol histograms (`deep_ll`, `deep_dist`, `widest`).  What the payloads reach is asserted on the CPU
(test_deflate_limits.py), where the kernel's staging is also restated with each of these paths broken: the members differ.

A member's words are the memory's: which tokens cross into a third word depends on where the member begins, modulo 4.
The first member of a launch begins at a multiple of 4, so every payload also goes behind a member whose size is 1, 2 and 3
modulo 4 (sizes: the host twin's)."""
import numpy as np
import pytest

from npore_amd import _lib
import deflate_limit_cases as dlc
from test_bam_deflate import content, host_member
from test_bam_match import ALL, any_content
from test_gpu_bam_match import ctx, device_members, want_member     # noqa: F401 (ctx: the module's fixture)

pytestmark = pytest.mark.gpu
P = dlc.P


def members_in_front():
    """{size modulo 4: payload} of the contents the suite has"""
    out = {}
    for kind, new in ALL:
        data = any_content(kind, new, P)
        out.setdefault(len(want_member(data)) % 4, data)
    return out


def check(ctx, data, phase, n_head, payloads, n_tail, mode=2):
    mem, head, tail, pos = device_members(ctx, data, phase, mode)
    assert (len(head), len(mem), len(tail)) == (n_head, len(payloads), n_tail)
    assert head == data[:n_head] and tail == data[len(data) - n_tail:] and pos == phase + len(data)
    for k, (m, payload) in enumerate(zip(mem, payloads)):
        want = want_member(payload) if mode == 2 else host_member(payload)
        assert len(m) == len(want) and m == want, (k, len(m), len(want), int(np.nonzero(np.frombuffer(m, np.uint8) != np.frombuffer(want, np.uint8))[0][0]) if len(m) == len(want) else -1)


@pytest.mark.parametrize("name", dlc.NAMES)
def test_limits_equal_host_twin(ctx, name):
    payload, pr = dlc.case(name)
    assert pr["written"] and len(want_member(payload)) == pr["match_member"]
    check(ctx, payload[-3:] + payload + payload + payload[:5], P - 3, 3, [payload, payload], 5)
    check(ctx, payload, 0, 0, [payload], 0)
    check(ctx, payload[17:] + payload + payload[:9], 17, P - 17, [payload], 9)
    front = members_in_front()
    assert sorted(front) == [0, 1, 2, 3]
    for r in (1, 2, 3):                                             # the member begins at every address modulo 4
        check(ctx, front[r] + payload, 0, 0, [front[r], payload], 0)


def test_limits_between_other_members(ctx):
    """Match members at the limits between ordinary ones, a stored and a literals-only member (emit_literal_member out of
    emit_match_kernel) among them: the staging words and the hash tables are clean from member to member."""
    parts = [content("golden", P), dlc.payload("wide"), content("uniform", P), dlc.payload("deep_ll"), content("one", P),
             dlc.payload("deep_dist"), dlc.payload("widest")]
    assert len(want_member(parts[2])) == P + 31                     # stored
    data = b"".join(parts)
    check(ctx, data, 0, 0, parts, 0)
    check(ctx, parts[0][1:] + data, 1, P - 1, parts, 0)


def test_mode_1_on_limits(ctx):
    parts = [dlc.payload(name) for name in dlc.NAMES]
    check(ctx, b"".join(parts), 0, 0, parts, 0, mode=1)
    check(ctx, b"".join(parts), 0, 0, parts, 0)                     # ... and with matches again, on the same context


def test_too_little_room_is_refused_and_the_next_call_is_right(ctx):
    """The caller's room, not the kernels': the debug entry's own buffers always hold n // P + 1 members of P + 31 bytes, so
    place_deflate_kernel's `no room` and emit_fragments' `more members than max_members` cannot be reached through it."""
    lib = _lib.load()
    parts = [dlc.payload("wide"), dlc.payload("deep_ll")]
    data = b"".join(parts)
    comp = sum(len(want_member(p)) for p in parts)
    src = np.frombuffer(data, np.uint8)
    head, tail, info = np.full(P, 0xEE, np.uint8), np.full(P, 0xEE, np.uint8), np.full(5, -7, np.int64)
    for members_cap, sizes_cap in ((comp - 1, 2), (comp, 1)):
        out, sizes = np.full(comp, 0xEE, np.uint8), np.full(2, 0xEEEEEEEE, np.uint32)
        rc = lib.npore_debug_deflate_device_mode(ctx.handle, src.ctypes.data, len(data), 0, out.ctypes.data, members_cap, sizes.ctypes.data, sizes_cap,
                                                 head.ctypes.data, tail.ctypes.data, info.ctypes.data, 2)
        assert rc != 0 and "the members need more room than the caller gave" in _lib.last_error()
        assert (out == 0xEE).all() and (sizes == 0xEEEEEEEE).all() and (info == -7).all() and (head == 0xEE).all()
        check(ctx, data, 0, 0, parts, 0)
