"""The inflate routes of nxz_batch_decompress and the environment that names each of them (the engine reads these knobs
at every call): one place for the tests that run a batch on every route."""
import contextlib
import os

# a stream per workgroup with everything in LDS (what every batch gets; what that kernel does not do it hands to the
# stream-per-wavefront kernel), the same with pieces of 250 bits of which a wavefront walks every one that must go again
# ("wg-128": the name is from when the launcher's default piece was not 128 bits -- it is now, so that setting only
# repeated "wg"; the name stays so that the tests keep theirs); a stream per lane; the same with the fixed-code-only
# kernel in front (which hands a batch with a dynamic block in it back to the first); a stream per wave with its window in
# LDS, with the target buffer as its window (what mid-size batches get), and that with the jobs taken in the order of
# their lengths (what batches of more than one round of wavefronts get); every stream cut inside its first block into up
# to 32 pieces (what small batches get: nxz_inflate_cut.hip), or 3
ROUTES = ["wg", "wg-128", "lanes", "lanes-fixed", "waves", "waves-global-window", "waves-by-length", "cut", "cut-3"]


@contextlib.contextmanager
def inflate_route(route):
    """set the environment for one route, and put it back"""
    assert route in ROUTES
    old = os.environ.get("NXZ_INFLATE_LANES_MIN")
    os.environ["NXZ_INFLATE_LANES_MIN"] = "32" if route.startswith("lanes") else "1000000000"
    os.environ["NXZ_LANES_FIXED"] = "2" if route == "lanes-fixed" else "0"
    os.environ["NXZ_INFLATE_CUT"] = "1" if route.startswith("cut") else "0"
    os.environ["NXZ_INFLATE_WG"] = "1" if route.startswith("wg") else "0"
    if route == "wg-128":
        os.environ["NXZ_WG_PMIN"] = "250"
        os.environ["NXZ_WG_COOP"] = "1024"
    if route == "cut-3":
        os.environ["NXZ_INFLATE_CUT_PIECES"] = "3"
    if route in ("waves-global-window", "waves-by-length"):
        os.environ["NXZ_INFLATE_LDS_MAX"] = "0"
    if route == "waves-by-length":                  # (the jobs in the order of their lengths, as batches beyond one round of wavefronts go)
        os.environ["NXZ_INFLATE_ORDER"] = "1"
    try:
        yield route
    finally:
        os.environ.pop("NXZ_INFLATE_ORDER", None)
        os.environ.pop("NXZ_INFLATE_WG", None)
        os.environ.pop("NXZ_WG_PMIN", None)
        os.environ.pop("NXZ_WG_COOP", None)
        os.environ.pop("NXZ_INFLATE_CUT", None)
        os.environ.pop("NXZ_INFLATE_CUT_PIECES", None)
        os.environ["NXZ_INFLATE_LANES_MIN"] = old if old is not None else "32"
        os.environ.pop("NXZ_INFLATE_LDS_MAX", None)
        os.environ.pop("NXZ_LANES_FIXED", None)
