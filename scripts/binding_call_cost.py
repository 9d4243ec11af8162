"""Host cost of one library call through the ctypes binding, no GPU needed: mdg_lars_multi with zero chunks returns 0 before it
touches a device.  Times it with every argument hand-wrapped against an untyped handle (the binding before the header typed it)
and with plain values against the typed handle of _lib.lib().   python scripts/binding_call_cost.py [calls]  -> one JSON line"""
import ctypes, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madrigal_amd import _lib

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
typed = _lib.lib()
untyped = ctypes.CDLL(_lib.LIB_PATH)                    # a second handle: its function objects carry no argtypes
tables, n, ws, nbytes, stream = [4096 * (i + 1) for i in range(6)], 0, 1 << 20, 1 << 16, 0
vp, c64 = ctypes.c_void_p, ctypes.c_int64


def hand_wrapped():
    _lib.check(untyped.mdg_lars_multi(vp(tables[0]), vp(tables[1]), vp(tables[2]), vp(tables[3]), vp(tables[4]), vp(tables[5]), c64(n), c64(n),
                                      vp(ws), ctypes.c_size_t(nbytes), vp(stream)), "mdg_lars_multi")


def plain_values():
    _lib.call("mdg_lars_multi", tables[0], tables[1], tables[2], tables[3], tables[4], tables[5], n, n, ws, nbytes, stream)


def per_call_us(fn) -> float:
    best = float("inf")
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        best = min(best, (time.perf_counter() - t0) / calls * 1e6)
    return best


a, b = per_call_us(hand_wrapped), per_call_us(plain_values)
print(json.dumps({"entry": "mdg_lars_multi (zero chunks, 11 arguments)", "calls": calls, "repeats": 5, "statistic": "best of the repeats",
                  "hand_wrapped_untyped_us_per_call": round(a, 3), "plain_values_typed_us_per_call": round(b, 3), "ratio": round(b / a, 3)}))
