"""Case list and inputs of test_batched_physics_gpu.py, read without a GPU by test_batched_physics_cpu.py."""
import torch

# (path, grid, dtype): which loss pass the UNBATCHED call and the batched call take on the grid
#   generic : 2D below 34 x 34 or without 16-byte lanes -- pi_residual_sq_kernel either way
#   tile    : 2D from 34 x 34 on with 16-byte lanes -- pi_res2d_tile_kernel ((40, 100): ragged edge tiles)
#   3d      : the unbatched call runs the brick pass where it applies, the batched call the generic kernel
GRIDS = [
    ("generic", (3, 5), torch.float64),
    ("generic", (7, 6), torch.float64),
    ("generic", (33, 64), torch.float32),
    ("tile", (34, 36), torch.float64),
    ("tile", (40, 100), torch.float32),
    ("tile", (64, 96), torch.float32),
    ("3d", (7, 6, 8), torch.float64),
    ("3d", (9, 12, 16), torch.float32),
]
FORMS = ("shared", "per_sample")          # Q [36] / Q [B, 36]
BATCHES = (1, 2, 3, 5)
FRAMES = (1, 3, 9)                        # F: frames with a residual; the trajectory has F + 2

# loss value: two passes that differ only in the order of the float64 sums (the bounds of
# test_physics_loss_2d_tile_pass_equals_generic_pass / test_physics_loss_3d_brick_pass_equals_generic_pass)
LOSS_TOL = {torch.float32: 1e-6, torch.float64: 1e-13}


def cases():
    """every grid x block form x weighting; B and F walk their sets so that each value meets each path"""
    out = []
    for path, shape, dtype in GRIDS:
        for form in FORMS:
            for weighted in (True, False):
                i = len(out)
                out.append(dict(path=path, shape=shape, dtype=dtype, form=form, weighted=weighted,
                                B=BATCHES[(i + i // 4) % 4], F=FRAMES[(i + i // 12) % 3], seed=100 + i))
    return out


def case_id(c):
    return "{}-{}-{}-{}-{}-B{}-F{}".format(c["path"], "x".join(map(str, c["shape"])), str(c["dtype"]).split(".")[1], c["form"],
                                           "weighted" if c["weighted"] else "plain", c["B"], c["F"])


def family(c):
    """the reference's equation the case is scored against (oracle/restatement.py::physics_loss_reference)"""
    return "gs3d" if len(c["shape"]) == 3 else ("gs2d" if c["dtype"] == torch.float32 else "lo2d")


def trajectory(c):
    """[F+2, B, 2, *S] uniform in [0, 1) on the CPU: far from a solution, so every loss is far from zero"""
    return torch.rand((c["F"] + 2, c["B"], 2) + tuple(c["shape"]), dtype=c["dtype"],
                      generator=torch.Generator().manual_seed(c["seed"]))


def make_cell(c):
    import percnn_amd as pa
    if len(c["shape"]) == 3:
        return pa.RCNNCell(3, 2, dx=0.5, dt=0.1, mu_up=0.2, dtype=c["dtype"])
    return pa.gs2d_cell() if c["dtype"] == torch.float32 else pa.lo2d_cell()


def block(cell, fam, b=0):
    """equation block of member b: b = 0 is the reference's coefficient set; other members differ in dt, the diffusivities
    and the reaction coefficients"""
    from percnn_amd import physics
    w, dt = cell.W_laplace.weight, cell.dt * (1.0 + 0.25 * b)
    if fam == "lo2d":
        D, a = 0.1 + 0.02 * b, 1.0 + 0.1 * b
        return physics.pde_block(w, dt, D, D, {"u": a, "uuu": -1.0, "uvv": -1.0, "uuv": 1.0, "vvv": 1.0},
                                 {"uuu": -1.0, "uvv": -1.0, "v": a, "uuv": -1.0, "vvv": -1.0})
    Du, Dv, f, k = (2e-5, 5e-6, 1 / 25, 3 / 50) if fam == "gs2d" else (0.2, 0.1, 0.025, 0.055)
    Du, f, k = Du * (1.0 + 0.1 * b), f + 0.005 * b, k + 0.003 * b
    return physics.pde_block(w, dt, Du, Dv, {"1": f, "u": -f, "uvv": -1.0}, {"uvv": 1.0, "v": -(f + k)})


def blocks(c, cell):
    """Q of the case: [36] (member 0's) or [B, 36]"""
    fam = family(c)
    if c["form"] == "shared":
        return block(cell, fam)
    return torch.stack([block(cell, fam, b) for b in range(c["B"])])
