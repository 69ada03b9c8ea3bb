#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: a complete pipeline of a fixture on WORLD_SIZE ranks (torch.distributed; all ranks may share GPU 0 with gloo:
VFT_SAME_DEVICE=1) - the NJ sweeps AND the lanes of the subtree schedule split over the ranks (vft_comm).  Every rank prints
`rank crc32(tree) bytes lane_allgathers lane_bytes loglk <the TreeLogLk lines as hex floats: treeLogLk's pair likelihoods are split over the ranks too> end`.  run_pipeline_ranks.py <fixture name>"""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import torch.distributed as dist
    import golden_util as G
    name = sys.argv[1]
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = 0 if os.environ.get("VFT_SAME_DEVICE") else int(os.environ.get("LOCAL_RANK", "0"))
    from veryfasttree_amd import HipProfileOps
    from veryfasttree_amd.backend import TorchComm, nj_newick, last_lane_exchange
    comm = None
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group(os.environ.get("VFT_BACKEND", "nccl"))
        comm = TorchComm(dist, local)
    d = G.load(name)
    run, _, names = G.reference_run(d)
    make = lambda n, L: HipProfileOps(n, L, run.n_codes, run.dtype, max_nodes=3 * n, device=local)
    ml = "ml_nni" in run.kwargs or "mllen" in run.kwargs
    tree = nj_newick(make, d["codes"], names, me_lengths=True, comm=comm, return_loglk=ml, **run.kwargs)
    loglk = []
    if ml:
        tree, loglk = tree
    calls, nbytes = last_lane_exchange()
    # (one write per rank: the ranks share a pipe, and print() hands text and newline over separately - lines interleaved mid-way)
    sys.stdout.write("rank %d crc %d bytes %d lane_allgathers %d lane_bytes %d loglk %s end\n" % (comm.rank if comm else 0, zlib.crc32(tree.encode()), len(tree), calls, nbytes,
                                                                                                ",".join(float(x).hex() for x in loglk)))
    sys.stdout.flush()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
