"""Hand-worked NO_WAIT epochs with their expected decisions, shared by the CPU
test of the replay (test_nowait_ref.py) and the GPU parity test
(test_gpu_nowait.py).  Each case: (name, txns, held, rc, conflict); held is
a list of (key, acctype) or None; conflict uses N for ACCESS_NONE."""
from deneva_amd import ACCESS_NONE as N
from deneva_amd import RC_ABORT as AB
from deneva_amd import RC_RCOK as OK
from deneva_amd import RD, SCAN, WR, XP

KATS = [
    ("sh_sh", [[(7, RD)], [(7, RD)]], None, [OK, OK], [N, N]),
    ("sh_then_ex", [[(7, RD)], [(7, WR)]], None, [OK, AB], [N, 0]),
    ("ex_then_sh", [[(7, WR)], [(7, RD)]], None, [OK, AB], [N, 0]),
    ("ex_then_ex", [[(7, WR)], [(7, WR)]], None, [OK, AB], [N, 0]),
    # txn 1 aborts at its second request and frees row 2 again for txn 2
    ("abort_releases", [[(1, WR)], [(2, WR), (1, RD)], [(2, WR)]], None, [OK, AB, OK], [N, 1, N]),
    # NO_WAIT keeps no owner list: a txn conflicts with its own earlier request
    ("self_sh_ex", [[(5, RD), (5, WR)]], None, [AB], [1]),
    ("self_ex_sh", [[(5, WR), (9, RD), (5, RD)]], None, [AB], [2]),
    ("self_ex_ex", [[(5, WR), (5, WR)]], None, [AB], [1]),
    ("self_sh_sh", [[(5, RD), (5, RD)]], None, [OK], [N]),
    # a self-conflicting txn leaves no trace either
    ("self_then_other", [[(5, RD), (5, WR)], [(5, WR)]], None, [AB, OK], [1, N]),
    # an earlier request may conflict with somebody else first
    ("other_before_self", [[(3, WR)], [(3, RD), (5, RD), (5, WR)]], None, [OK, AB], [N, 0]),
    ("xp_is_ex", [[(4, XP)], [(4, RD)], [(6, RD)], [(6, XP)]], None, [OK, AB, OK, AB], [N, 0, N, 0]),
    ("scan_is_sh", [[(4, SCAN)], [(4, RD)], [(4, SCAN)], [(4, WR)]], None, [OK, OK, OK, AB], [N, N, N, 0]),
    ("held_ex", [[(8, RD)], [(8, WR)], [(9, WR)]], [(8, WR)], [AB, AB, OK], [0, 0, N]),
    ("held_sh", [[(8, RD)], [(1, RD), (8, WR)], [(8, SCAN)]], [(8, RD)], [OK, AB, OK], [N, 1, N]),
    # a row is EX-held if any of its entries is EX
    ("held_mixed", [[(8, RD)], [(3, RD)]], [(8, RD), (8, XP), (3, SCAN), (3, RD)], [AB, OK], [0, N]),
    # the conflict is the first failing request, found only at the fixed point:
    # txn 2's request 0 is blocked by txn 1 (which aborts) while its request 1
    # is killed by txn 0
    ("first_of_two", [[(1, WR), (2, WR)], [(1, RD), (3, WR)], [(3, RD), (2, RD)]], None,
     [OK, AB, AB], [N, 0, 1]),
    ("zero_length", [[], [(1, WR)], [], [(1, RD)], []], None, [OK, OK, OK, AB, OK], [N, N, N, 0, N]),
]
