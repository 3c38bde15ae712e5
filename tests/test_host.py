"""CPU-only checks: the C ABI library loads and exports every declared symbol, host logic, module surface."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import lss_ref as ref
import lss_carla_amd as L
from lss_carla_amd import _lib, ops
from lss_carla_amd import synthetic as syn

HEADERS = [os.path.join(REPO, "include", h) for h in ("lss_hip.h", "lss_convs.h", "lss_simbev.h")]


def _declared():
    text = "".join(open(h).read() for h in HEADERS)
    return set(re.findall(r"^\s*(?:int|int32_t|int64_t|size_t|const char\*)\s+(lss_\w+)\s*\(", text, re.M))


def test_header_declarations_match_binding():
    assert _declared() == set(_lib.SIGNATURES), _declared() ^ set(_lib.SIGNATURES)


def test_library_loads_and_exports_all_symbols():
    lib = _lib.load()  # built by __graft_entry__.build(); raises if missing
    for name in _declared():
        assert hasattr(lib, name), name
    assert lib.lss_abi_version() == _lib.ABI_VERSION
    assert lib.lss_error_string(0) == b"success"
    assert b"invalid" in lib.lss_error_string(-1)
    # host-side argument validation (no device work): NULL pointers are rejected
    assert lib.lss_geometry_cells(None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert lib.lss_ceiling_store(None, 16, 1, 0, None, None, None) == -1
    assert lib.lss_csr_scratch_bytes(4096, 100) == 256 + 8 * 100  # scan partials (aligned) + unsorted keys
    assert lib.lss_debug_checks() == (1 if os.environ.get("LSS_DEBUG", "0") == "1" else 0)


def test_debug_library_loads_and_exports_all_symbols():
    """liblss_hip_debug.so (LSS_DEBUG=1: device-side index checks) exposes the same ABI."""
    dbg = _lib.open_library(_lib.DEBUG_LIB_PATH)
    for name in _declared():
        assert hasattr(dbg, name), name
    assert dbg.lss_debug_checks() == 1
    assert dbg.lss_debug_status(None, 0) == -1  # NULL output rejected without touching a device


def test_build_lists_every_source_and_watches_every_header(tmp_path, monkeypatch):
    """A csrc file the build does not know fails here, not as a missing symbol at load time."""
    import glob

    from lss_carla_amd import build

    csrc = os.path.join(os.path.dirname(build.__file__), "csrc")
    assert sorted(build.SOURCES) == sorted(glob.glob(os.path.join(csrc, "*.hip")))
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    headers = glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(REPO, "include", "*.h"))
    assert headers and set(headers) <= set(build.HEADERS), set(headers) - set(build.HEADERS)
    # up_to_date() really looks at each of them: a library older than any one source or header is stale
    out = tmp_path / "lib.so"
    out.write_bytes(b"")
    newest = max(os.path.getmtime(f) for f in build.SOURCES + build.HEADERS + [build.__file__])
    os.utime(out, (newest + 1, newest + 1))
    assert build.up_to_date(str(out))
    real = os.path.getmtime
    for f in build.SOURCES + build.HEADERS:
        monkeypatch.setattr(os.path, "getmtime", lambda p, f=f: newest + 2 if p == f else real(p))
        assert not build.up_to_date(str(out)), f


def test_gridspec_matches_reference_quantiser_constants():
    gs = ops.GridSpec.from_conf(syn.grid_conf())
    dx, bx, nx = ref.gen_dx_bx([-50.0, 50.0, 0.5], [-50.0, 50.0, 0.5], [-10.0, 10.0, 20.0])
    assert gs.nx == tuple(nx.tolist())
    assert np.array_equal(np.array(gs.lo, dtype=np.float32), (bx - dx / np.float32(2)).astype(np.float32))
    assert gs.ncells(8) == 8 * 200 * 200


def test_module_surface_and_state_dict():
    gc, dac = syn.grid_conf(), syn.data_aug_conf()
    m = L.compile_model(gc, dac, outC=1)
    assert isinstance(m, L.LiftSplatShoot)
    sd = m.state_dict()
    keys = list(sd)
    assert keys[:4] == ["dx", "bx", "nx", "frustum"]
    assert m.dx.requires_grad is False and m.nx.dtype == torch.long
    assert m.D == 41 and m.camC == 64 and m.downsample == 16 and m.use_quickcumsum is True
    np.testing.assert_array_equal(m.frustum.detach().numpy(), ref.create_frustum((128, 352), gc["dbound"]).numpy())
    for k in ("camencode.trunk._conv_stem.weight", "camencode.trunk._blocks.15._project_conv.weight",
              "camencode.trunk._blocks.1._expand_conv.weight", "camencode.trunk._blocks.0._se_reduce.bias",
              "camencode.trunk._fc.weight", "camencode.up1.conv.4.running_var", "camencode.depthnet.weight",
              "bevencode.conv1.weight", "bevencode.layer2.0.downsample.1.weight", "bevencode.up2.4.bias"):
        assert k in sd, k
    assert "camencode.trunk._blocks.0._expand_conv.weight" not in sd  # expand ratio 1 block
    assert len(m.camencode.trunk._blocks) == 16
    assert sum(p.numel() for p in m.parameters()) == 14313575
    assert m.camencode.depthnet.out_channels == 41 + 64
    # zero_init_residual of the torchvision trunk parts
    assert m.bevencode.layer1[0].bn2.weight.abs().sum() == 0
    assert m.bevencode.layer1[0].bn1.weight.sum() == 64
    # BevEncode parameter order = the reference's (conv1 first)
    names = [n for n, _ in m.bevencode.named_parameters()]
    assert names[0] == "conv1.weight" and names[1] == "bn1.weight"


def test_efficientnet_static_same_padding():
    m = L.compile_model(syn.grid_conf(), syn.data_aug_conf(), outC=1)
    t = m.camencode.trunk
    assert isinstance(t._conv_stem.static_padding, torch.nn.ZeroPad2d)
    assert t._conv_stem.static_padding.padding == (0, 1, 0, 1)
    assert t._blocks[3]._depthwise_conv.static_padding.padding == (1, 2, 1, 2)
    assert t._blocks[4]._depthwise_conv.padding == (2, 2)
    # endpoints on a 128x352 image: the depthnet output is 8x22
    m.eval()
    with torch.no_grad():
        feats = m.camencode.get_eff_depth(torch.randn(1, 3, 128, 352))
    assert feats.shape == (1, 512, 8, 22)


def test_cpu_forward_fails_loudly():
    gc = syn.grid_conf()
    m = L.compile_model(gc, syn.data_aug_conf((64, 176)), outC=1)
    rig = syn.make_rig(1, 2, (64, 176))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(1, 2, 3, 64, 176), **rig)


def test_synthetic_rig_shapes():
    rig = syn.make_rig(3, 6, (128, 352))
    assert rig["rots"].shape == (3, 6, 3, 3) and rig["post_trans"].shape == (3, 6, 3)
    # val-mode crop of the 224x480 image to 128x352: resize 352/480, crop_h = 164 - 128
    assert np.isclose(rig["post_rots"][0, 0, 0, 0].item(), 352 / 480)
    assert rig["post_trans"][0, 0].tolist() == [0.0, -36.0, 0.0]
    dn = syn.make_depthnet_out(1, 1, 41, 8, 22)
    assert dn.shape == (1, 105, 8, 22)


def test_bench_gpus_flag_launches_one_rank_per_gpu(monkeypatch):
    """`bench.py --gpus N` without a torchrun environment re-launches itself as N ranks (torchrun on
    127.0.0.1) before touching the GPU, and exits with the job's status."""
    import importlib.util
    import sys as _sys
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    monkeypatch.setattr(bench.subprocess, "call", fake_call)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "8", "--steps", "3"])
    args = bench.parse()
    with pytest.raises(SystemExit) as e:
        bench.maybe_launch_ranks(args)
    assert e.value.code == 7
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=8" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "8", "--steps", "3"] and seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    monkeypatch.setenv("WORLD_SIZE", "8")  # under torchrun: no second launch
    assert bench.maybe_launch_ranks(args) is None
    assert args.config == "c3" and args.batch == 8 and args.mode == "train" and args.bev_layout == "nhwc"


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_bench", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_plain_run_measures_the_headline_only(monkeypatch):
    """Without --full every extra measurement is off (roofline child runs, profile steps, CPU baseline,
    MIOpen's per-process find); --full restores today's defaults, and explicit switches still apply."""
    import sys as _sys
    bench = _load_bench()
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, "")
    assert (a.profile_steps, a.in_graph_prof, a.pmc_traffic, a.cpu_baseline, a.miopen_find) == (0, 0, 0, 0, 0)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert (a.profile_steps, a.in_graph_prof, a.pmc_traffic, a.cpu_baseline, a.miopen_find) == (20, 1, 1, 1, 1)
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--full", "--cpu-baseline", "0", "--miopen-find", "0",
                                       "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.cpu_baseline, a.miopen_find, a.pmc_traffic, a.dump_outputs) == (0, 0, 1, "d")
    monkeypatch.setattr(_sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_arrays(tmp_path, monkeypatch):
    """--dump-outputs: float32 arrays of the step's value and of the gradients in the optimizer's order (not
    the updated parameters); an array over the cap is the same seeded sample on every call."""
    import torch
    bench = _load_bench()

    class Step:  # what collect_outputs reads of a captured train_step.TrainStep
        params = [torch.arange(6, dtype=torch.float64).reshape(2, 3), torch.full((4,), 7.0)]
        graph_grads = [torch.ones(2, 3), torch.arange(4.0)]

    arrays = bench.collect_outputs(Step(), torch.tensor(0.25, dtype=torch.bfloat16), "train")
    assert sorted(arrays) == ["grads", "loss"] and all(a.dtype == np.float32 for a in arrays.values())
    assert arrays["loss"].shape == () and float(arrays["loss"]) == 0.25
    assert arrays["grads"].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 2, 3]
    Step.graph_grads = None  # eager: the parameters' own .grad, zeros where a parameter has none
    Step.params[0].grad = torch.full((2, 3), 2.0, dtype=torch.float64)
    assert bench.collect_outputs(Step(), torch.tensor(0.0), "train")["grads"].tolist() == [2] * 6 + [0] * 4
    fwd = bench.collect_outputs(bench.FwdStep(None, ()), torch.ones(2, 1, 3, 3), "fwd")
    assert list(fwd) == ["preds"] and fwd["preds"].shape == (2, 1, 3, 3)

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 5)
    Step.params = [torch.arange(100.0)]
    Step.graph_grads = [torch.arange(100.0) * 2]
    a, b = (bench.collect_outputs(Step(), torch.tensor(0.0), "train") for _ in range(2))
    assert a["grads"].shape == (5,) and np.array_equal(a["grads"], b["grads"])
    assert len(set(a["grads"].tolist())) > 1 and all(g % 2 == 0 and 0 <= g < 200 for g in a["grads"].tolist())
    bench.write_outputs(a, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["grads.npy", "loss.npy"]
    assert np.array_equal(np.load(tmp_path / "out" / "grads.npy"), a["grads"])


def test_bench_dumped_step_starts_from_the_initial_state():
    """restore_initial: parameters, Adam state (in place: same tensors) and the generators as at the
    start, so the step after it repeats the run's first step bit for bit (CPU: no atomics)."""
    import torch
    from lss_carla_amd.train_step import TrainStep
    bench = _load_bench()
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Dropout(0.5), torch.nn.Linear(7, 1))
    params = list(net.parameters())
    opt = torch.optim.Adam(params, lr=1e-2, weight_decay=1e-7)
    x, y = torch.randn(4, 5), torch.randn(4, 1)
    step = TrainStep(net, (x,), y, torch.nn.functional.mse_loss, opt, params, amp_dtype=None)
    assert bench.step_params(step) == params and bench.step_params(bench.FwdStep(net, (x,))) == []
    snap = [p.detach().clone() for p in params]
    torch.manual_seed(11)
    first = step().detach().clone()
    g1, p1 = [p.grad.clone() for p in params], [p.detach().clone() for p in params]
    for _ in range(3):
        step()
    state_ids = [id(v) for st in opt.state.values() for v in st.values()]
    bench.restore_initial(step, snap, 11)
    assert all(torch.equal(p, s) for p, s in zip(params, snap))
    assert state_ids == [id(v) for st in opt.state.values() for v in st.values()]
    assert all(float(torch.as_tensor(v).abs().max()) == 0 for st in opt.state.values() for v in st.values())
    again = step()
    assert torch.equal(again, first) and all(torch.equal(p.grad, g) for p, g in zip(params, g1))
    assert all(torch.equal(p, q) for p, q in zip(params, p1))  # the fresh Adam state gives the first update


def test_bench_keeps_the_committed_miopen_databases(tmp_path):
    """MIOpen gets a working copy of tuning/miopen/db: same content, refreshed when the source is newer."""
    bench = _load_bench()
    src = tmp_path / "tuning" / "miopen" / "db"
    src.mkdir(parents=True)
    (src / "a.udb.txt").write_text("one\n")
    db, cache = bench.miopen_dirs(str(tmp_path))
    assert db == os.path.join(cache, "db") and open(os.path.join(db, "a.udb.txt")).read() == "one\n"
    with open(os.path.join(db, "a.udb.txt"), "a") as fh:  # MIOpen appends to its copy: kept, source untouched
        fh.write("two\n")
    bench.miopen_dirs(str(tmp_path))
    assert open(os.path.join(db, "a.udb.txt")).read() == "one\ntwo\n" and (src / "a.udb.txt").read_text() == "one\n"
    (src / "a.udb.txt").write_text("three\n")
    t = os.path.getmtime(os.path.join(db, "a.udb.txt")) + 10
    os.utime(src / "a.udb.txt", (t, t))
    bench.miopen_dirs(str(tmp_path))
    assert open(os.path.join(db, "a.udb.txt")).read() == "three\n"


def test_bench_runs_from_a_tree_it_cannot_write(tmp_path, monkeypatch):
    """Where tuning/miopen/cache cannot be made (a read-only checkout; here: a file is in its place),
    MIOpen's working copy and kernel cache go to a directory of this user and checkout under the
    system's temporary directory; the conftest restatement agrees with bench.py."""
    import tempfile
    import conftest
    bench = _load_bench()
    repo = tmp_path / "ro"
    (repo / "tuning" / "miopen" / "db").mkdir(parents=True)
    (repo / "tuning" / "miopen" / "db" / "a.ufdb.txt").write_text("one\n")
    (repo / "tuning" / "miopen" / "cache").write_text("")
    (tmp_path / "t").mkdir()
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path / "t"))
    db, cache = bench.miopen_dirs(str(repo))
    assert cache.startswith(str(tmp_path / "t") + os.sep) and db == os.path.join(cache, "db")
    assert open(os.path.join(db, "a.ufdb.txt")).read() == "one\n"
    assert conftest._miopen_dirs(str(repo)) == (db, cache)
    os.rename(repo, tmp_path / "ro2")  # another checkout, another directory
    repo = tmp_path / "ro2"
    cache2 = bench.miopen_dirs(str(repo))[1]
    assert cache2 != cache and cache2.startswith(str(tmp_path / "t") + os.sep)
    monkeypatch.setattr(tempfile, "tempdir", str(repo / "tuning" / "miopen" / "cache" / "x"))  # nowhere to write
    assert bench.miopen_dirs(str(repo)) == (str(repo / "tuning" / "miopen" / "db"),
                                            str(repo / "tuning" / "miopen" / "cache"))


def test_hip_adam_only_for_plain_cuda_adam():
    """optim.supported: the lss_clip_adam path is never taken for CPU tensors or other optimizers."""
    import torch
    from lss_carla_amd import optim
    ps = [torch.zeros(4, requires_grad=True), torch.zeros(3, requires_grad=True)]
    for p in ps:
        p.grad = torch.ones_like(p)
    assert not optim.supported(torch.optim.Adam(ps, lr=1e-3), ps)  # CPU tensors
    assert not optim.supported(torch.optim.SGD(ps, lr=1e-3), ps)


def test_pointwise_conv_size_guard():
    """pointwise_conv routes to lss_pw_conv / lss_pw_wrw only inside the index limits those kernels check
    (EINVAL past them); larger activations stay on the framework conv."""
    from lss_carla_amd import efficientnet as E
    assert E._pw_fits(48, 512, 105, 176)
    assert not E._pw_fits(4096, 1152, 192, 704)        # N * C * HW >= 2^31
    assert E._pw_fits(1, 2**20, 1, 2047) and not E._pw_fits(1, 2**20, 1, 2048)


# ---- alignment backstop of the conv-stack C ABI (include/lss_convs.h): checked on the host before any
# HIP call, so made-up addresses that are never dereferenced exercise it without a GPU
_A = 0x10000  # a 16-B aligned fake address; arrays handed out 4 KiB apart
_EINVAL = -1


def _fake(i: int, off: int = 0) -> int:
    return _A + 0x1000 * i + off


def _bn_fwd(lib, x, y, dtype, layout, N, C, HW, res=None, gamma=None):
    st = _fake(8)
    return lib.lss_bn_fwd2(x, res, dtype, layout, N, C, HW, gamma or _fake(2), _fake(3), 1e-5, 0.1, _fake(4), _fake(5),
                           _fake(6), 1, 1, _fake(7), st, st + 4 * C, st + 8 * C, st + 12 * C, y, None, None)


def _bn_bwd(lib, dy, x, y, dx, dtype, layout, N, C, HW, dres=None):
    st = _fake(8)
    return lib.lss_bn_bwd2(dy, x, y, dtype, layout, N, C, HW, st + 8 * C, st + 12 * C, st, st + 4 * C, 1, 1, _fake(7),
                           _fake(9), _fake(10), _fake(11), dx, dres, None, None)


def test_bn_entry_points_refuse_bad_sizes_and_unaligned_pointers():
    lib = _lib.load()
    x, y, dy, dx = _fake(0), _fake(1), _fake(12), _fake(13)
    F32, BF16, NCHW, NHWC = _lib.F32, _lib.BF16, _lib.NCHW, _lib.NHWC
    # aligned pointers, bad sizes
    for N, C, HW in ((0, 8, 24), (2, 0, 24), (2, 8, 0), (2, 8, -4), (1 << 15, 1 << 10, 1 << 6)):
        assert _bn_fwd(lib, x, y, BF16, NCHW, N, C, HW) == _EINVAL
        assert _bn_bwd(lib, dy, x, y, dx, BF16, NCHW, N, C, HW) == _EINVAL
    # channels-last needs C % 8 == 0 (and 256 % (C / 8) == 0)
    for C in (12, 4, 24):
        assert _bn_fwd(lib, x, y, BF16, NHWC, 2, C, 15) == _EINVAL
        assert _bn_bwd(lib, dy, x, y, dx, BF16, NHWC, 2, C, 15) == _EINVAL
        assert lib.lss_bn_bwd_rank1(_fake(14), _fake(15), x, 2, C, 15, _fake(8) + 8 * C, _fake(8) + 12 * C, _fake(8),
                                    _fake(8) + 4 * C, 1, 1, _fake(7), _fake(9), _fake(10), _fake(11), dx,
                                    None) == _EINVAL
    assert _bn_fwd(lib, x, y, 2, NCHW, 2, 8, 24) == _EINVAL  # unknown dtype
    # good sizes, one activation pointer off the width the kernels pick for (dtype, layout, HW):
    # bf16 NCHW HW % 8 == 0 -> 16 B; HW % 8 == 4 -> 8 B; fp32 HW % 4 == 0 -> 16 B; NHWC -> 16 B
    cases = [(BF16, NCHW, 8, 24, (2, 4, 8)), (BF16, NCHW, 8, 12, (2, 4)), (F32, NCHW, 8, 24, (4, 8)),
             (BF16, NHWC, 16, 15, (2, 4, 8)), (F32, NHWC, 16, 15, (4, 8)), (BF16, NCHW, 8, 15, (1,)),
             (F32, NCHW, 8, 15, (2,))]
    for dtype, layout, C, HW, offs in cases:
        for off in offs:
            assert _bn_fwd(lib, x + off, y, dtype, layout, 2, C, HW) == _EINVAL, (dtype, layout, HW, off)
            assert _bn_fwd(lib, x, y + off, dtype, layout, 2, C, HW) == _EINVAL
            assert _bn_fwd(lib, x, y, dtype, layout, 2, C, HW, res=_fake(14, off)) == _EINVAL
            for k in range(5):
                p = [dy, x, y, dx, _fake(14)]
                p[k] += off
                assert _bn_bwd(lib, p[0], p[1], p[2], p[3], dtype, layout, 2, C, HW, dres=p[4]) == _EINVAL, k
    assert _bn_fwd(lib, x, y, BF16, NCHW, 2, 8, 24, gamma=_fake(2, 2)) == _EINVAL  # fp32 arrays: 4 B
    st = _fake(8)
    for k in (2, 16):  # x, dx of the rank-1 backward
        a = [_fake(14), _fake(15), x, 2, 16, 15, st + 128, st + 192, st, st + 64, 1, 1, _fake(7), _fake(9), _fake(10),
             _fake(11), dx, None]
        a[k] += 2
        assert lib.lss_bn_bwd_rank1(*a) == _EINVAL


def test_se_and_head1_entry_points_refuse_bad_sizes_and_unaligned_pointers():
    lib = _lib.load()
    f = [_fake(i) for i in range(16)]

    def se_fwd(x, y, N, C, HW, sq):
        return lib.lss_se_fwd(x, N, C, HW, f[2], f[3], f[4], f[5], sq, f[6], f[7], f[8], f[9], y, None)

    def se_bwd(dy, x, dx, N, C, HW, sq):
        return lib.lss_se_bwd(dy, x, N, C, HW, f[2], f[4], sq, f[7], f[9], f[10], f[11], f[12], f[13], f[14], dx, None)

    for N, C, HW, sq in ((2, 8, 6, 2), (2, 2056, 4, 2), (2, 8, 8, 65), (0, 8, 8, 2), (2, 8, 8, 0)):  # bad sizes
        assert se_fwd(f[0], f[1], N, C, HW, sq) == _EINVAL
        assert se_bwd(f[15], f[0], f[1], N, C, HW, sq) == _EINVAL
    for off in (2, 4):  # four bf16 per access: 8 B
        assert se_fwd(f[0] + off, f[1], 2, 8, 8, 2) == _EINVAL and se_fwd(f[0], f[1] + off, 2, 8, 8, 2) == _EINVAL
        for k in range(3):
            p = [f[15], f[0], f[1]]
            p[k] += off
            assert se_bwd(p[0], p[1], p[2], 2, 8, 8, 2) == _EINVAL

    for P, C in ((0, 64), (10, 12), (10, 0), (10, 24 * 8), (10, 1024)):  # rows of C / 8 16-B vectors, 64 % (C / 8) == 0
        assert lib.lss_head1_fwd2(f[0], f[2], None, P, C, None, f[1], None) == _EINVAL
        assert lib.lss_head1_bwd2(f[0], f[3], f[2], P, C, None, f[1], f[4], None) == _EINVAL
    for off in (2, 4, 8):
        assert lib.lss_head1_fwd2(f[0] + off, f[2], None, 10, 64, None, f[1], None) == _EINVAL
        assert lib.lss_head1_fwd(f[0] + off, f[2], None, 10, 64, f[1], None) == _EINVAL
        assert lib.lss_head1_bwd2(f[0] + off, f[3], f[2], 10, 64, None, f[1], f[4], None) == _EINVAL
        assert lib.lss_head1_bwd2(f[0], f[3], f[2], 10, 64, None, f[1] + off, f[4], None) == _EINVAL
        assert lib.lss_head1_bwd(f[0], f[3], f[2], 10, 64, f[1] + off, f[4], None) == _EINVAL
    assert lib.lss_head1_fwd2(f[0], f[2], None, 10, 64, None, f[1] + 1, None) == _EINVAL  # y / dy: bf16 elements
    assert lib.lss_head1_bwd2(f[0], f[3] + 1, f[2], 10, 64, None, f[1], f[4], None) == _EINVAL


def test_dwconv_entry_points_refuse_bad_sizes_and_unaligned_pointers():
    lib = _lib.load()
    f = [_fake(i) for i in range(8)]
    good = (2, 8, 6, 8, 3, 1, 1, 1, 6, 8)  # N, C, Hi, Wi, K, stride, pad_top, pad_left, Ho, Wo

    def calls(x, y, w, geo, dtype=_lib.BF16):
        N = geo[0]
        return (lib.lss_dwconv_fwd(x, dtype, w, *geo, y, None),
                lib.lss_dwconv_bwd_data(y, dtype, w, *geo, x, None),
                lib.lss_dwconv_bwd_weight(x, y, dtype, *geo, N, f[3], None),
                lib.lss_dwconv_bwd_weight2(x, y, dtype, *geo, N, f[3], f[4], f[5], None))

    for bad in ((2, 8, 6, 8, 4, 1, 1, 1, 6, 8), (2, 8, 6, 8, 3, 3, 1, 1, 6, 8), (0, 8, 6, 8, 3, 1, 1, 1, 6, 8),
                (2, 8, 6, 8, 3, 1, 1, 1, 0, 8), (1 << 12, 1 << 12, 16, 16, 3, 1, 1, 1, 16, 16)):
        assert calls(f[0], f[1], f[2], bad) == (_EINVAL,) * 4, bad
    assert calls(f[0], f[1], f[2], good, dtype=2) == (_EINVAL,) * 4
    for off in (2, 4, 8):
        assert calls(f[0] + off, f[1], f[2], good) == (_EINVAL,) * 4
        assert calls(f[0], f[1] + off, f[2], good) == (_EINVAL,) * 4
        assert calls(f[0] + off, f[1], f[2], good, dtype=_lib.F32) == (_EINVAL,) * 4


# ---- kernel-selection arms (tests/arm_cases.py): the queries are host-only, so the table's coverage of the
# arms is proved here; tests/test_gpu_dispatch_arms.py then runs every case on the GPU
import ctypes  # noqa: E402

import arm_cases as A  # noqa: E402


def _dims(B, N, D, H, W):
    return ctypes.byref(ops.make_dims(B, N, D, H, W))


def _dw_arm(lib, pas, dtype, c):
    Ho, Wo = A.dw_out(c)
    pl, _, pt, _ = c.pads
    a = _lib.DwArm()
    assert lib.lss_dwconv_arm(pas, dtype, c.N, c.C, c.H, c.W, c.K, c.S, pt, pl, Ho, Wo, A.dw_groups(c),
                              ctypes.byref(a)) == 0, c
    assert a.pb >= (1 if a.family < 4 else 0) and a.seg in ((8, 4) if a.family < 2 else (0,)), (c, a.seg, a.pb)
    assert not (a.banded and a.pb != 1), c
    return A.dw_arm_name(a.family, a.seg, a.banded, a.pb)


def test_arm_tables_cover_every_splat_and_lift_arm():
    lib = _lib.load()
    # splat backward: each case hits the arm it names; per row dtype the cases hit exactly the arms of the header
    assert len(A.BWD_ARM_NAMES) == 6 and set(A.BWD_D) == {c.D for c in A.BWD_CASES}
    for code, dt in ((_lib.F32, A.F32), (_lib.BF16, A.BF16)):
        hit = {}
        for c in A.BWD_CASES:
            arm = lib.lss_splat_bwd_arm(code, _dims(*c.shape[:2], c.D, *c.shape[2:]))
            assert arm == A.bwd_arm_of(c, dt), (c, A.BWD_ARM_NAMES[arm])
            hit.setdefault(arm, set()).add(c.Z)
        assert set(hit) == A.BWD_ARMS[dt]
        assert all(z == {1, 2} for z in hit.values()), hit  # every arm with one and with two z bins
        for shape, lo, hi, split in A.BWD_BOUNDARIES:
            a, b = (lib.lss_splat_bwd_arm(code, _dims(*shape[:2], D, *shape[2:])) for D in (lo, hi))
            assert (a != b) == split and a >= 0 and b >= 0, (shape, lo, a, b)
            assert {(shape, lo), (shape, hi)} <= {(c.shape, c.D) for c in A.BWD_CASES}
        assert lib.lss_splat_bwd_arm(code, _dims(1, 2, 256, 2, 4)) == A.REG4
        assert lib.lss_splat_bwd_arm(code, _dims(1, 2, 257, 2, 4)) == A.EUNSUPPORTED
        assert lib.lss_splat_bwd_arm(code, _dims(1, 2, 0, 2, 4)) == _EINVAL
    assert A.BWD_ARMS[A.F32] | A.BWD_ARMS[A.BF16] == set(range(6))
    assert lib.lss_splat_bwd_arm(2, _dims(1, 2, 41, 2, 4)) == _EINVAL and lib.lss_splat_bwd_arm(0, None) == _EINVAL
    assert len(A.BWD_COMBOS) == 16
    # lift prep
    for BN, H, W in A.PREP_SHAPES:
        assert {lib.lss_lift_prep_arm(_dims(1, BN, D, H, W)) for D in A.PREP_D} == A.PREP_ARMS
        for D, ni in A.PREP_D.items():
            assert lib.lss_lift_prep_arm(_dims(1, BN, D, H, W)) == ni and D <= 4 * ni, D
        for lo, hi in A.PREP_BOUNDARIES:
            assert A.PREP_D[lo] != A.PREP_D[hi]
        assert lib.lss_lift_prep_arm(_dims(1, BN, 257, H, W)) == A.EUNSUPPORTED
    assert lib.lss_lift_prep_arm(None) == _EINVAL and len(A.PREP_COMBOS) == 4
    # splat forward: its 12 instantiations are its arguments themselves
    assert {(layout, mode, out) for layout, mode, out, _ in A.FWD_CASES} == A.FWD_ARMS and len(A.FWD_ARMS) == 12
    assert {z for *_, z in A.FWD_CASES} == {1, 2}
    for Z in (1, 2):
        cells = A.fwd_geometry(Z)[1]
        kept = cells[cells >= 0]
        B = A.FWD_DIMS[0]
        assert 0 < (cells < 0).mean() < 0.5 and kept.max() < B * Z * 64
        assert np.bincount(kept).max() >= A.FWD_CROWD


def test_arm_table_covers_every_depthwise_arm():
    lib = _lib.load()
    hit = {}
    for c in A.DW_CASES:
        for pas, want in ((A.DW_FWD, c.fwd), (A.DW_BWD_DATA, c.bwd_data), (A.DW_BWD_WEIGHT, c.bwd_weight)):
            got = {_dw_arm(lib, pas, dt, c) for dt in (_lib.F32, _lib.BF16)}
            assert got == {want}, (c, pas, got)
            hit.setdefault((pas, c.K, c.S), set()).add(want)
    for pas in (A.DW_FWD, A.DW_BWD_DATA, A.DW_BWD_WEIGHT):
        for K in (3, 5):
            for S in (1, 2):
                assert hit[pas, K, S] == A.dw_arms(pas, K, S), (pas, K, S, hit[pas, K, S] ^ A.dw_arms(pas, K, S))
    families = {a.split("/")[0] for arms in hit.values() for a in arms}
    assert families == set(A.DW_FAMILIES)
    # the stride-2 parities on both odd-by-even maps; one and several image groups; N = 1 and 3
    for hw in ((5, 6), (6, 5)):
        for K in (3, 5):
            assert {c.bwd_data for c in A.DW_CASES if (c.H, c.W, c.K) == (*hw, K)} == A.dw_arms(A.DW_BWD_DATA, K, 2)
    assert {A.dw_groups(c) for c in A.DW_CASES} == {1, 2} and {1, 3} <= {c.N for c in A.DW_CASES}
    assert {A.dw_groups(c) for c in A.DW_FOLD_OFF} == {1, 2}
    # a covered right edge is what keeps a Wo % 4 == 0 plane on the LDS kernels
    off = [c for c in A.DW_CASES if "not covered" in c.note]
    assert {(c.K, c.S) for c in off} == {(3, 2), (5, 2)}
    assert all(A.dw_out(c)[1] == 8 and c.fwd == "reg" and c.bwd_weight == "reg" for c in off)
    # stride-1 backward-data chooses by the mirrored shape
    assert any(c.S == 1 and c.fwd != c.bwd_data and c.bwd_data == "reg" for c in A.DW_CASES)
    assert any(c.S == 1 and c.fwd == "reg" and c.bwd_data.startswith("lds") for c in A.DW_CASES)
    a = _lib.DwArm()
    assert lib.lss_dwconv_arm(3, 0, 2, 8, 6, 8, 3, 1, 1, 1, 6, 8, 1, ctypes.byref(a)) == _EINVAL  # pass
    assert lib.lss_dwconv_arm(0, 2, 2, 8, 6, 8, 3, 1, 1, 1, 6, 8, 1, ctypes.byref(a)) == _EINVAL  # dtype
    assert lib.lss_dwconv_arm(0, 0, 2, 8, 6, 8, 4, 1, 1, 1, 6, 8, 1, ctypes.byref(a)) == _EINVAL  # K
    assert lib.lss_dwconv_arm(2, 0, 2, 8, 6, 8, 3, 1, 1, 1, 6, 8, 3, ctypes.byref(a)) == _EINVAL  # groups > N
    assert lib.lss_dwconv_arm(0, 0, 2, 8, 6, 8, 3, 1, 1, 1, 6, 8, 1, None) == _EINVAL


def _room(got, want, rtol, atol):
    want = np.asarray(want, dtype=np.float64)
    return float((np.abs(np.asarray(got, dtype=np.float64) - want) / (atol + rtol * np.abs(want))).max())


def test_arm_references_fp32_margins():
    """The bars of the arm tests leave a plain fp32 evaluation of each reference formula at least 4x room at
    the largest case: a kernel that accumulates in fp32 in any order can meet them."""
    big = max(A.BWD_CASES, key=lambda c: (c.D, np.prod(c.shape)))
    assert big.D == 256
    ins = A.bwd_inputs(big)
    rooms = {"splat_bwd": _room(A.bwd_reference(*ins, dtype=np.float32), A.bwd_reference(*ins), **A.F32_TOL)}
    x = A.prep_input(*A.PREP_SHAPES[-1][:1], 256, *A.PREP_SHAPES[-1][1:])
    rooms["lift_prep"] = _room(A.prep_reference(x, 256, np.float32)[0], A.prep_reference(x, 256)[0], **A.F32_TOL)
    cells = A.fwd_geometry(2)[1]
    depth, ctx, rows = A.fwd_inputs(2)
    rooms["splat_fwd"] = _room(A.fwd_reference(cells, 2, depth, ctx, dtype=np.float32),
                               A.fwd_reference(cells, 2, depth, ctx), **A.F32_TOL)
    rooms["splat_fwd_lifted"] = _room(A.fwd_reference(cells, 2, rows=rows, dtype=np.float32),
                                      A.fwd_reference(cells, 2, rows=rows), **A.F32_TOL)
    import torch.nn.functional as Fn
    tall = max(A.DW_CASES, key=lambda c: c.H)
    most = max(A.DW_CASES, key=lambda c: c.N * c.H * c.W)
    for name, c in (("dw_tall", tall), ("dw_groups", most)):
        x, w, dy = A.dw_inputs(c, A.F32)
        outs = []
        for dt in (torch.float32, torch.float64):
            xr, wr = x.detach().to(dt).clone().requires_grad_(True), w.detach().to(dt).clone().requires_grad_(True)
            y = Fn.conv2d(Fn.pad(xr, c.pads), wr, stride=c.S, groups=c.C)
            y.backward(dy.to(dt))
            outs.append((y.detach().numpy(), xr.grad.numpy(), wr.grad.numpy()))
        tol, wtol = A.dw_tols(A.F32)
        rooms[name] = max(_room(outs[0][0], outs[1][0], **tol), _room(outs[0][1], outs[1][1], **tol))
        rooms[name + "_dw"] = _room(outs[0][2], outs[1][2], **wtol)
    # batch norm: the largest case of each family, bf16-exact inputs (the register and cluster kernels' dtype),
    # fp32 arithmetic in numpy's pairwise order and one element after the other, against every bar
    half = {"k": 0.0, "k_sq": 0.0}
    for fam, cases in _bn_families().items():
        c = max(cases, key=lambda c: c.N * c.H * c.W)
        combo = A.BnCombo("swish", False, "y")
        ins = A.bn_inputs(c, A.BF16, combo)
        want = A.bn_reference(ins, combo, A.BF16)
        for order in ("pairwise", "sequential"):
            got = A.bn_reference(ins, combo, A.BF16, ft=np.float32, order=order, fed=want)
            r = _bn_rooms(got, want, ins, combo)
            print("bn", fam, c.N * c.H * c.W, order, {n: round(v, 3) for n, v in r.items()})
            # the maps' bars are the project's, not chosen here: 4x room in numpy's order; y through statistics
            # summed one element after the other over 32,800 elements still meets its bar (0.87 of it)
            maps = max(r.pop(n) for n in ("y", "dx", "dres"))
            assert maps <= (0.25 if order == "pairwise" else 1.0), (fam, order, maps)
            rooms["bn_%s_%s" % (fam, order)] = max(r.values())
            r = _bn_rooms(got, want, ins, combo, k=A.BN_K // 2)
            half["k"] = max([half["k"]] + [r[n] for n in ("mean", "run_mean", "dbeta", "dgamma")])
            r = _bn_rooms(got, want, ins, combo, k_sq=A.BN_K_SQ // 2)
            half["k_sq"] = max([half["k_sq"]] + [r[n] for n in ("rstd", "scale", "shift", "run_var")])
    assert min(half.values()) > 0.25, half  # BN_K and BN_K_SQ are the smallest powers of two that do
    print({k: round(v, 4) for k, v in rooms.items()})
    assert all(v <= 0.25 for v in rooms.values()), rooms


# ---- batch norm (tests/arm_cases.py's BN section; tests/test_gpu_bn_arms.py runs it on the GPU)
def _bn_families():
    fams = {}
    for c in A.BN_CASES:
        for name in {c.f32, c.bf16} | set(c.bwd or ()):
            fams.setdefault(name.split("<")[0], []).append(c)
    return fams


def _bn_rooms(got, want, ins, combo, k=A.BN_K, k_sq=A.BN_K_SQ):
    """Largest |got - want| / bar of each per-channel output and each fp32 map of one evaluation."""
    bars = dict(A.bn_fwd_bars(want, ins, k, k_sq), **A.bn_bwd_bars(want, ins, combo, k))
    bars.update({n: A.bn_map_bar(want[n], A.F32) for n in ("y", "dx", "dres")})
    return {n: float((np.abs(got[n].astype(np.float64) - want[n]) / bars[n]).max()) for n in bars}


def _bn_arm(lib, pas, dtype, c, act="none"):
    a = _lib.BnArm()
    assert lib.lss_bn_arm(pas, dtype, c.layout, c.N, c.C, c.H * c.W, A.ACT[act], c.G, int(c.sync),
                          ctypes.byref(a)) == 0, c
    assert a.launches == {"nhwc": 3, "two_pass": 2}.get(A.BN_FAMILIES[a.family], 1), c
    assert a.blocks == (c.G if c.layout == 1 else c.C * c.G) and a.chunks == 0, c
    return A.bn_arm_name(a.family, a.v, a.it, a.relu)


def test_arm_table_covers_every_batch_norm_arm():
    lib = _lib.load()
    for pas in (A.BN_FWD, A.BN_BWD):
        for code, dt in ((_lib.F32, A.F32), (_lib.BF16, A.BF16)):
            hit = set()
            for c in A.BN_CASES:
                for combo in A.bn_combos(c, pas):
                    got = _bn_arm(lib, pas, code, c, combo.act)
                    assert got == A.bn_case_arm(c, dt, pas, combo.act), (c, pas, dt, got)
                    hit.add(got)
            assert hit == A.bn_arms(pas, dt), (pas, dt, hit ^ A.bn_arms(pas, dt))
    assert lib.lss_bn_arm(0, 0, 0, 2, 3, 8, 0, 1, 0, None) == _EINVAL and _lib.BnArm().family == 0
    assert len(A.BN_FAMILIES) == 7  # LSS_BN_ARM_FAMILIES
    # each bound of the rule: its two neighbours are in the table and land on different arms
    notes = [c.note for c in A.BN_CASES]
    for lo, hi, dt, pas in A.BN_BOUNDARIES:
        a, b = (next(c for c in A.BN_CASES if c.note == n and c.layout == 0) for n in (lo, hi))
        assert lo in notes and hi in notes
        assert A.bn_case_arm(a, dt, pas) != A.bn_case_arm(b, dt, pas), (lo, hi)
    one = [c for c in A.BN_CASES if c.layout == 0 and c.G == 1]
    cnt = lambda c: c.N * c.H * c.W // (8 if c.H * c.W % 8 == 0 else 4)  # noqa: E731
    assert {1023, 1024, 1025, 1280, 1281, 2047, 2048, 2049} <= {cnt(c) for c in one if c.H * c.W % 8 == 0}
    assert {1023, 1024, 1025, 2048, 2049} <= {cnt(c) for c in one if c.H * c.W % 8 == 4}
    # every register instantiation has a case whose vectors per image (>= 3) do not divide the block
    for arm in ("fused_reg<8,4>", "fused_reg<8,5>", "fused_reg<8,8>", "fused_reg<4,4>", "fused_reg<4,8>"):
        per = [c.H * c.W // int(arm[10]) for c in one if c.bf16 == arm]
        assert any(p >= 3 and 256 % p for p in per), (arm, per)
    # the cluster's backward families differ from the forward's between 1024 and 2304 blocks
    assert any(c.bwd and c.bwd[1] != c.bf16 for c in A.BN_CASES)
    # two-pass: every V with uneven groups and one image a group, the second lap of the fold, an empty group
    for v in (8, 4, 1):
        tp = [c for c in A.BN_CASES if c.bf16 == "two_pass<%d>" % v and c.f32 == c.bf16 and not c.sync]
        assert any(c.N % c.G for c in tp) and any(c.G == c.N for c in tp), v
    assert any(c.G > 64 and c.layout == 0 for c in A.BN_CASES) and any(c.G > c.N and c.layout == 0 for c in A.BN_CASES)
    # NHWC: octets a row below, at and above a wave; rows below a pass, off and on the unrolled pass; group counts
    nh = [c for c in A.BN_CASES if c.layout == 1]
    assert {c.C for c in nh} == {8, 16, 64, 512, 2048} and {1, 2, 17, 1025} == {c.G for c in nh}
    for C in (8, 16, 64, 512, 2048):
        step, rows = 256 // (C // 8), {c.N * c.H * c.W for c in nh if c.C == C}
        assert any(m % (4 * step) for m in rows) and any(m % (4 * step) == 0 for m in rows), C
        assert step == 1 or any(m < step for m in rows), C
    assert any(c.G > c.N * c.H * c.W for c in nh)
    # bad pass, dtype, layout, sizes, activation, group counts
    a = ctypes.byref(_lib.BnArm())
    good = (0, 1, 0, 4, 3, 8, 0, 2, 1)
    assert lib.lss_bn_arm(*good, a) == 0
    for i, bad in ((0, 3), (0, -1), (1, 2), (2, 2), (3, 0), (4, 0), (5, 0), (5, -8), (6, 3), (7, 0)):
        args = list(good)
        args[i] = bad
        assert lib.lss_bn_arm(*args, a) == _EINVAL, (i, bad)
    assert lib.lss_bn_arm(0, 1, 0, 1 << 15, 1 << 10, 1 << 6, 0, 1, 0, a) == _EINVAL  # N C HW >= 2^31
    assert lib.lss_bn_arm(0, 1, 1, 2, 24, 8, 0, 1, 0, a) == _EINVAL   # NHWC: 256 % (C / 8) != 0
    assert lib.lss_bn_arm(0, 1, 1, 2, 16, 8, 0, 4096, 0, a) == 0
    assert lib.lss_bn_arm(1, 1, 1, 2, 16, 8, 0, 4097, 0, a) == _EINVAL  # NHWC: at most 4096 groups
    assert lib.lss_bn_arm(2, 1, 1, 2, 16, 8, 0, 0, 0, a) == 0  # eval does not read ngroups
    x, y, dy, dx = _fake(0), _fake(1), _fake(12), _fake(13)
    st = _fake(8)
    # the entry points agree on 4097 groups (made-up addresses: refused before any launch)
    assert lib.lss_bn_fwd2(x, None, 1, 1, 2, 16, 8, _fake(2), _fake(3), 1e-5, 0.1, None, None, None, 0, 4097, _fake(7),
                           st, st + 64, st + 128, st + 192, y, None, None) == _EINVAL
    assert lib.lss_bn_bwd2(dy, x, y, 1, 1, 2, 16, 8, st + 128, st + 192, st, st + 64, 0, 4097, _fake(7), _fake(9), None,
                           None, dx, None, None, None) == _EINVAL
    # the backward of swish with a residual does not exist: refused, not computed without the residual
    assert lib.lss_bn_bwd2(dy, x, y, 1, 0, 2, 3, 8, st + 24, st + 36, st, st + 12, 2, 1, _fake(7), _fake(9), None, None,
                           dx, _fake(14), None, None) == _EINVAL
    # lss_bn_groups' choice is what the through-Python cases assume
    for c in A.BN_CASES:
        if c.py:
            assert lib.lss_bn_groups(c.N, c.C, c.H * c.W, c.layout) == c.G, c
    assert lib.lss_bn_groups(2, 3, 64 * 128, 0) == 2 and lib.lss_bn_groups(3, 3, 8 * 683, 0) == 2  # ngroups 1: ABI only


def test_bn_eval_cases_cover_every_eval_arm():
    """tests/test_gpu_bn_eval.py's CASES (read from its source: the module needs a GPU to import) reach V in
    {8, 4, 1} x dtype for NCHW, NHWC, several chunks a channel and more units than the 1,024 blocks."""
    import ast
    src = open(os.path.join(REPO, "tests", "test_gpu_bn_eval.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "CASES")
    cases = ast.literal_eval(node.value)
    lib, hit, over = _lib.load(), set(), set()
    for layout, (N, C, H, W) in cases:
        for code in (_lib.F32, _lib.BF16):
            a = _lib.BnArm()
            assert lib.lss_bn_arm(A.BN_EVAL, code, int(layout == "nhwc"), N, C, H * W, 0, 1, 0, ctypes.byref(a)) == 0
            assert a.launches == 1 and a.it == 0 and a.relu == 0
            hit.add((A.bn_arm_name(a.family, a.v, 0, 0), code))
            if a.family == A.BN_FAMILIES.index("eval_nchw") and C * a.chunks > a.blocks:
                over.add("nchw")
            if a.family == A.BN_FAMILIES.index("eval_nhwc") and a.blocks == 1024:
                over.add("nhwc")
            if a.chunks > 1:
                over.add("chunks")
    want = {("eval_nchw<%d>" % v, code) for v in (4, 1) for code in (_lib.F32, _lib.BF16)}
    want |= {("eval_nchw<8>", _lib.BF16), ("eval_nhwc", _lib.F32), ("eval_nhwc", _lib.BF16)}  # fp32 never takes V 8
    assert hit == want, hit ^ want
    assert over == {"nchw", "nhwc", "chunks"}


def test_bn_reference_is_batch_norm():
    """arm_cases.bn_reference against F.batch_norm + autograd in fp64, on cases of every layout and activation."""
    import torch.nn.functional as Fn
    picks = [c for c in A.BN_CASES if c.note in ("V 1", "groups of 1, 2, 2", "15 rows < 32 a pass")]
    assert len(picks) >= 3
    for c in picks:
        for combo in (A.BnCombo("none", True, "y"), A.BnCombo("swish", False, "y"), A.BnCombo("relu", True, "y")):
            ins = A.bn_inputs(c, A.F32, combo)
            ref = A.bn_reference(ins, combo, A.F32)
            t = lambda a: torch.from_numpy(a.reshape(c.C, c.N, -1).transpose(1, 0, 2).copy())  # noqa: E731
            x = t(ins["x"]).requires_grad_(True)
            w, b = (torch.from_numpy(ins[k]).requires_grad_(True) for k in ("gamma", "beta"))
            r = t(ins["res"]).requires_grad_(True) if combo.res else None
            rm, rv = torch.from_numpy(ins["rm"].copy()), torch.from_numpy(ins["rv"].copy())
            z = Fn.batch_norm(x, rm, rv, w, b, training=True, momentum=A.BN_MOM, eps=A.BN_EPS)
            z = z + r if combo.res else z
            y = {"none": z, "relu": Fn.relu(z), "swish": Fn.silu(z)}[combo.act]
            y.backward(t(ins["dy"]))
            back = lambda g: g.detach().numpy().transpose(1, 0, 2).reshape(c.C, -1)  # noqa: E731
            # (the reference's backward starts from fp32-rounded statistics: 2^-24 relative)
            for got, want, tol in ((ref["y"], back(y), 1e-12), (ref["run_mean"], rm.numpy(), 1e-12),
                                   (ref["run_var"], rv.numpy(), 1e-12), (ref["dx"], back(x.grad), 1e-5),
                                   (ref["dbeta"], b.grad.numpy(), 1e-5), (ref["dgamma"], w.grad.numpy(), 1e-5)):
                np.testing.assert_allclose(got, want, rtol=tol, atol=tol)
            if combo.res:
                np.testing.assert_allclose(ref["dres"], back(r.grad), rtol=1e-12, atol=1e-12)


def test_bn_bars_notice_a_left_out_element_and_the_recompute_cap_holds():
    """For every case, dtype and combination: a reference that leaves the last element of each (channel, group)
    range out of its sums misses the bar on save_mean and on dbeta or dgamma: in every channel where the builder
    pinned the range ends; on save_mean in 99 % of the channels and on dbeta or dgamma in some channel otherwise. The pinned ends are at least one standard
    deviation off their channel's mean. And the elements the ReLU recompute arm may leave out of dx stay under
    the cap."""
    for c in A.BN_CASES:
        lasts = [b for _, b in A.bn_ranges(c)]
        for dt in (A.F32, A.BF16):
            for combo in A.bn_combos(c, A.BN_BWD):
                ins = A.bn_inputs(c, dt, combo)
                ref = A.bn_reference(ins, combo, dt)
                cut = A.bn_reference(ins, combo, dt, drop=lasts)
                fb, bb = A.bn_fwd_bars(ref, ins), A.bn_bwd_bars(ref, ins, combo)
                seen = np.abs(cut["mean"] - ref["mean"]) > fb["mean"]
                # (unpinned: a last element that happens to equal K, the sums' shift, adds nothing to them)
                assert seen.all() if A.bn_pinned(c) else seen.mean() >= 0.99, (c, dt, combo)
                miss = (np.abs(cut["dbeta"] - ref["dbeta"]) > bb["dbeta"]) | (np.abs(cut["dgamma"] - ref["dgamma"]) > bb["dgamma"])
                assert miss.all() if A.bn_pinned(c) else miss.any(), (c, dt, combo, miss)
                if A.bn_pinned(c):
                    ends = np.unique(np.array(A.bn_ranges(c)).reshape(-1))
                    off = np.abs(ins["x"][:, ends] - ref["mean"][:, None]) * ref["rstd"][:, None]
                    assert off.min() >= 1.0 and np.abs(ins["dy"][:, ends]).min() >= 1.0, (c, off.min())
                near = A.bn_near_zero(ref, combo)
                assert near.sum() <= A.BN_RECOMPUTE_CAP * near.size, (c, dt, int(near.sum()))
                assert combo.y == "null" or not near.any()


# ---- squeeze-excite (tests/arm_cases.py's SE section; tests/test_gpu_se_arms.py runs it on the GPU)
def _se_arm(lib, pas, c, setting):
    prev = lib.lss_se_tails(setting)
    try:
        a = _lib.SeArm()
        assert lib.lss_se_arm(pas, c.N, c.C, c.HW, c.sq, ctypes.byref(a)) == 0, c
    finally:
        lib.lss_se_tails(prev)
    return a


def test_arm_table_covers_every_squeeze_excite_class():
    lib = _lib.load()
    up = lambda n, d: -(-n // d)  # noqa: E731
    for pas in (A.SE_FWD, A.SE_BWD):
        for setting in (A.SE_OFF, A.SE_DEFAULT, A.SE_FORCED):
            hit = {}
            for c in A.SE_CASES:
                a = _se_arm(lib, pas, c, setting)
                path, planes, ragged, one, chunk = A.se_class(pas, a)
                axes = hit.setdefault(path, dict(planes=set(), one_block=set(), chunks=set()))
                axes["planes"].add((planes, ragged))
                axes["one_block"].add(one)
                axes["chunks"].add(chunk)
                # the report against the rule restated: the routing, the grids, the planes a wave, the chunks
                limit = 4096 if pas == A.SE_BWD else 1024
                tails = setting != A.SE_OFF and c.N <= A.SE_BANK_IMAGES and (setting == A.SE_FORCED or c.C * c.sq <= limit)
                assert a.tails == int(tails) and a.launches == (2 if tails else 4), (c, pas, setting)
                n4 = up(c.N * c.C * c.HW // 4, 256)
                if tails:
                    assert a.cpb % 16 == 0 and a.bpi == up(c.C, a.cpb) and a.bpi <= max(1, 512 // c.N), c
                    assert (a.bpi - 1) * a.cpb < c.C and list(a.grid) == [c.N * a.bpi, n4, 0, 0], c
                    last = c.C - (a.bpi - 1) * a.cpb
                    assert (a.planes_max, a.planes_min) == (up(min(a.cpb, c.C), 16), last // 16), c
                    assert a.w2_chunks == (0 if pas else up(c.C, min(1024, 16384 // (c.sq + 1)))), c
                else:
                    mid = [c.N * up(c.C, 64)] * 2 if pas else [c.N * up(c.sq, 4), c.N * up(c.C, 256)]
                    assert list(a.grid) == [up(c.N * c.C, 4)] + mid + [n4] and (a.bpi, a.cpb) == (0, 0), c
                    assert a.w2_chunks == (0 if pas else up(c.C, 256)), c
                assert a.chunks64 == (up(c.C, 64) if pas else 0), c
            if setting == A.SE_DEFAULT:  # either path, each within what the header enumerates
                assert set(hit) == {"tails", "sequence"}
                for path, axes in hit.items():
                    want = A.se_classes(pas, path == "tails")
                    assert all(axes[k] <= want[k] for k in want), (pas, path, axes)
            else:  # one path (past the bank: the sequence), every class of it
                path = "tails" if setting else "sequence"
                want = A.se_classes(pas, setting != A.SE_OFF)
                assert hit[path] == want, (pas, setting, {k: hit[path][k] ^ want[k] for k in want})
                assert set(hit) == ({"tails", "sequence"} if setting else {"sequence"})
    # each bound of the rule: its two neighbours are in the table and fall in different classes
    for lo, hi, pas, setting in A.SE_BOUNDARIES:
        a, b = (A.se_class(pas, _se_arm(lib, pas, A.se_case(n), setting)) for n in (lo, hi))
        assert a != b, (lo, hi, a)
    by = lambda f: {f(c) for c in A.SE_CASES}  # noqa: E731
    assert {63, 64, 65, 192, 193, 256, 257, 1025, 2048} <= by(lambda c: c.C)
    assert {1, 2, 3, 4, 5, 15, 16, 17, 63, 64} <= by(lambda c: c.sq)
    assert {4, 8, 12, 252, 256, 260, 516} <= by(lambda c: c.HW) and max(by(lambda c: c.HW)) <= 516
    assert any(c.C % 16 for c in A.SE_CASES) and {1, 15, 16, 17, 33} == {n for n, _, _ in A.SE_WGRAD_CASES}
    for N, C, sq in A.SE_WGRAD_CASES:
        assert (2 * C * sq + sq + C) % 256
    assert any(2 * C * sq + sq + C <= 64 for _, C, sq in A.SE_WGRAD_CASES)  # one wave holds all four branches
    assert all(A.se_case(n) for n in A.SE_AUTOGRAD) and len(A.SE_AUTOGRAD) == 3
    # the query refuses what the entry points refuse
    a = ctypes.byref(_lib.SeArm())
    assert lib.lss_se_arm(0, 2, 8, 8, 2, a) == 0 and lib.lss_se_arm(1, 2, 2048, 4, 64, a) == 0
    for bad in ((2, 2, 8, 8, 2), (-1, 2, 8, 8, 2), (0, 2, 8, 6, 2), (0, 2, 2049, 4, 2), (1, 2, 8, 8, 65), (0, 0, 8, 8, 2),
                (1, 2, 8, 8, 0), (0, 2, 0, 8, 2), (0, 2, 8, 0, 2), (0, 1 << 15, 1 << 10, 1 << 6, 2)):
        assert lib.lss_se_arm(*bad, a) == _EINVAL, bad
    assert lib.lss_se_arm(0, 2, 8, 8, 2, None) == _EINVAL


def _se_eval_rooms(ins, ref, got):
    """|error| / bar of every stage of an evaluation that kept its values before the bf16 roundings: those are held
    to the fp32 part of the bar alone."""
    pre = lambda n, st: float((np.abs(got["pre_" + n].astype(np.float64) - st[0]) / st[1]).max())  # noqa: E731
    f, b = A.se_fwd_stages(ins, got), A.se_bwd_stages(ins, ref, got)
    r = {n: pre(n, f[n]) for n in ("m", "r", "h", "e")}
    r["sig"] = pre("sig", A.se_sig_stage(got["e"]))
    r.update({n: float(A.se_ratio(got[n], *b[n], False).max()) for n in ("t", "de", "dh_part", "dr", "dm")})
    r["dx"] = pre("dx", b["dx"])
    r.update(A.se_wgrad_rooms([ref[k].astype(np.float32) for k in ("de", "h", "dr", "m")], got))
    return r


def test_se_bars_leave_fp32_room_and_notice_a_left_out_term():
    """On every case: (1) an fp32 numpy evaluation of the contract -- numpy's pairwise sums or one term after the
    other, numpy's exp -- stays within a quarter of every bar, and passes the test the GPU buffers are put to; (2) the
    fp64 reference itself passes it; (3) a value with one term left out does not: the last element of every plane in m
    and t; per output the largest term of r (a channel), of e under sig (a j), of dh under dr (a channel), of dm (a j);
    the image of the largest term in each of the four gradients."""
    worst, shares = {}, []
    for c in A.SE_CASES:
        ins = A.se_inputs(c.N, c.C, c.HW, c.sq)
        ref = A.se_reference(ins)
        assert max(A.se_rooms(ins, ref, ref).values()) <= 1.0, c
        for n in A.SE_FWD_BF16 + ("sig",):
            assert np.array_equal(ref[n], ref[n].astype(np.float32)) and not (ref[n].astype(np.float32).view(np.uint32) & 0xFFFF).any()
        for order in ("pairwise", "sequential"):
            got = A.se_reference(ins, ft=np.float32, order=order, fed=ref)
            for n, v in _se_eval_rooms(ins, ref, got).items():
                worst[n] = max(worst.get(n, 0.0), v)
                assert v <= 0.25, (c, order, n, v)
            assert max(A.se_rooms(ins, got, ref).values()) <= 1.0, (c, order)
        # ---- one term left out
        x, dy = ins["x"], ins["dy"]
        w1, b1, w2, b2 = A.se_weights(ins)
        f, b = A.se_fwd_stages(ins, ref), A.se_bwd_stages(ins, ref, ref)
        N, sq = c.N, c.sq
        seen = lambda got, st, bf: A.se_ratio(got, *st, bf) > 1.0  # noqa: E731
        assert seen(A.rbf(f["m"][0] - x[..., -1] / c.HW), f["m"], True).all(), (c, "m")
        assert seen(b["t"][0] - (dy * x)[..., -1], b["t"], False).all(), (c, "t")
        top = lambda terms: np.take_along_axis(terms, np.abs(terms).argmax(axis=-1)[..., None], -1)[..., 0]  # noqa: E731
        assert seen(A.rbf(f["r"][0] - top(ref["m"][:, None, :] * w1[None])), f["r"], True).all(), (c, "r")
        gone = top(ref["h"][:, None, :] * w2[None])
        cut = A.rbf(A._sigmoid(A.rbf(f["e"][0] - gone)))
        sig_seen = A.se_sig_ratio(cut, *f["e"]) > 1.0
        # sig passes two bf16 roundings (e, then sig): a term shows for certain once it moves e by more than a bf16
        # step of e and, through the sigmoid's smallest slope on the way, sig by more than a bf16 step of sig
        ends = np.stack([f["e"][0], f["e"][0] - gone])
        step_e = 4 * A.bf16_half(A.rbf(np.abs(ends).max(axis=0)), np.inf)
        ends = np.concatenate([ends - step_e, ends + step_e])
        sg = A._sigmoid(ends)
        must = (sg * (1 - sg)).min(axis=0) * (np.abs(gone) - step_e) > 4 * A.bf16_half(A.rbf(sg.max(axis=0)), np.inf)
        assert sig_seen[must].all() and must.mean() >= 0.5, (c, "sig", must.mean(), sig_seen.mean())
        shares.append((A.se_id(c), round(float(must.mean()), 3), round(float(sig_seen.mean()), 3)))
        s = A._sigmoid(ref["r"])
        slope = s * (1 + ref["r"] * (1 - s))
        assert seen(b["dr"][0] - top(ref["de"][:, None, :] * w2.T[None]) * slope, b["dr"], False).all(), (c, "dr")
        assert seen(b["dm"][0] - top(ref["dr"][:, None, :] * w1.T[None]), b["dm"], False).all(), (c, "dm")
        fed4 = [ref[k].astype(np.float32).astype(np.float64) for k in ("de", "h", "dr", "m")]
        st = A.se_wgrad_stages(*fed4)
        de, h, dr, m = fed4
        terms = {"dw1": dr.T[:, None, :] * m.T[None], "db1": dr.T, "dw2": de.T[:, None, :] * h.T[None], "db2": de.T}
        for n, term in terms.items():
            # (a sum of N terms in sequence is allowed SE_ROOM N u of its summands: one of N equal terms shows while
            # SE_ROOM N^2 u < 1, N < 2048. The two cases at the counter bank's limit cannot shrink below 4096.)
            gone = top(term)  # (0 where a pooled mean of four is exactly 0: nothing to notice)
            assert (seen(st[n][0] - gone, st[n], False) | (gone == 0)).all() or c.N >= A.SE_BANK_IMAGES, (c, n)
    for N, C, sq in A.SE_WGRAD_CASES:
        fed4 = A.se_wgrad_inputs(N, C, sq)
        st = A.se_wgrad_stages(*fed4)
        for order in ("pairwise", "sequential"):
            got = A.se_wgrad_reference(*fed4, ft=np.float32, order=order)
            for n in st:
                assert float(A.se_ratio(got[n], *st[n], False).max()) <= 0.25, (N, C, sq, order, n)
    print({k: round(v, 3) for k, v in worst.items()}, shares)


def test_se_reference_is_squeeze_excite():
    """arm_cases.se_reference against the stock ops + autograd in fp64: the bf16 roundings move values by up to
    2^-8 relative, so this pins the formulas, not the bits."""
    import torch.nn.functional as Fn
    for note in A.SE_AUTOGRAD + ("C 65, sq 5",):
        c = A.se_case(note)
        ins = A.se_inputs(c.N, c.C, c.HW, c.sq)
        ref = A.se_reference(ins)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        x = t(ins["x"]).reshape(c.N, c.C, c.HW, 1).requires_grad_(True)
        w1, b1, w2, b2 = (t(w).requires_grad_(True) for w in A.se_weights(ins))
        hid = Fn.silu(Fn.conv2d(Fn.adaptive_avg_pool2d(x, 1), w1.reshape(c.sq, c.C, 1, 1), b1))
        y = x * torch.sigmoid(Fn.conv2d(hid, w2.reshape(c.C, c.sq, 1, 1), b2))
        y.backward(t(ins["dy"]).reshape(x.shape))
        for got, want in ((ref["y"], y.detach().reshape(c.N, c.C, c.HW)), (ref["dx"], x.grad.reshape(c.N, c.C, c.HW)),
                          (ref["dw1"], w1.grad), (ref["db1"], b1.grad), (ref["dw2"], w2.grad), (ref["db2"], b2.grad)):
            want = want.numpy()
            assert np.abs(got - want).max() <= 2e-2 * np.abs(want).max(), (note, np.abs(got - want).max())
