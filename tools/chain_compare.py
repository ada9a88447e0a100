"""Every call of the carrier-chain family (csrc/host/carr_chain.c) on the rows of three scenarios,
for the library GSS_LIB_PATH names (else the in-tree build): one sha256 per call and output array,
the hits included.  Two builds compute the same when their listings are equal
(profiles/refactor_chain/).

Scenarios: static at 2.6 MS/s, the circle motion file, and the integer carrier; four batches of
350 blocks each from next_deferred, every call with 1, 3 and 8 threads.

usage: [GSS_LIB_PATH=... GSS_ALLOW_LIB_OVERRIDE=1] python tools/chain_compare.py > listing.txt"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "gps-sdr-sim_amd"))
import gpssim_amd as G

DATA = os.path.join(REPO, "tests", "golden", "data")
NAV = os.path.join(DATA, "brdc3540.14n")
CIRCLE = os.path.join(DATA, "circle.csv")
LOC = (30.286502, 120.032669, 100.0)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scenario(kind):
    if kind == "static":
        return G.Scenario(NAV, llh=LOC, duration=300.0, samp_freq=2.6e6)
    if kind == "circle":
        return G.Scenario(NAV, motion_file=CIRCLE, duration=300.0)
    return G.Scenario(NAV, llh=LOC, duration=300.0, carrier="int")


def batch(tag, carr, blk, nch, chain, n, cint, threads):
    """Every call on one batch; returns the exact chain's end carriers."""
    def out(call, *arrays):
        print(f"{tag} t{threads} {call:28} {sha(*arrays)}")

    for ck in (False, True):
        b = blk.copy()
        end, cks = G.carr_chain(carr, b, nch, chain, n, carrier_int=cint, with_ck=ck,
                                threads=threads)
        out("carr_chain" + ("+ck" if ck else ""), end, b, *([cks] if ck else []))
    starts = G.carr_chain_guess(carr, blk, nch, chain, n, starts_only=True)
    gi = G.carr_chain_guess(carr, blk, nch, chain, n)
    out("carr_chain_guess starts", starts)
    out("carr_chain_guess", gi)
    out("carr_line_end", G.carr_line_end(carr, blk, nch, chain, n))
    spec = G.spec_host(starts, n, threads=threads).reshape(gi.shape)
    out("spec_host", starts, spec)                 # the starts completed in place, and the walks
    b = blk.copy()
    e, hit = G.carr_chain_spec(carr, b, nch, chain, n, gi, spec, threads=threads)
    out("carr_chain_spec", e, b, np.int64(hit))
    b = blk.copy()
    e, hit, anch = G.carr_chain_anchored(carr, b, nch, chain, n, gi, spec, threads=threads)
    out("carr_chain_anchored", e, b, np.int64(hit), anch)
    out("carr_anchors", G.carr_anchors(b, nch, n, gi, spec, threads=threads))
    rec = G.spec_records(gi, spec, n, threads=threads)
    out("spec_records", rec)
    b = blk.copy()
    e, hit = G.carr_chain_records(carr, b, nch, chain, n, rec, threads=threads)
    out("carr_chain_records", e, b, np.int64(hit))
    link = G.spec_links(nch, chain, n, gi, spec, threads=threads)
    out("spec_links", link)
    b = blk.copy()
    e, hit = G.carr_chain_linked(carr, b, nch, chain, n, gi, spec, link, threads=threads)
    out("carr_chain_linked", e, b, np.int64(hit))
    return end


def main():
    for kind in ("static", "circle", "intcarr"):
        s = scenario(kind)
        carr = s.carrier()
        for i in range(4):
            blk, nch, chain = s.next_deferred(350, threads=8)
            print(f"{kind}{i} rows {int(nch.sum())} resets {int(chain['reset'].sum())} "
                  f"input {sha(carr, blk, nch, chain)}")
            for threads in (1, 3, 8):
                end = batch(f"{kind}{i}", carr, blk, nch, chain, s.n_per_blk, s.carrier_int,
                            threads)
            carr = end


if __name__ == "__main__":
    main()
