"""Host-side checks of the measurement scripts (no GPU): they parse, and the PMC json bench.py quotes is what
scripts/make_pmc_json.py derives from the committed counter summary."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_and_extra_parse_their_arguments():
    for script in ('bench.py', os.path.join('scripts', 'bench_extra.py')):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), '--help'], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and 'usage' in r.stdout, (script, r.stderr[-500:])


def test_pmc_json_is_regenerated_from_the_committed_summary(tmp_path):
    out = tmp_path / 'pmc.json'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'make_pmc_json.py'),
                        os.path.join(ROOT, 'profiles', 'r04_pmc_summary.txt'), str(out),
                        os.path.join(ROOT, 'profiles', 'r04_kernel_stats_f16gpx3_serial.txt')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-500:]
    new, old = json.load(open(out)), json.load(open(os.path.join(ROOT, 'profiles', 'r04_pmc.json')))
    assert new['kernel_class'] == 'nt8' and new['hbm_bytes_per_launch'] == old['hbm_bytes_per_launch']
    for k in ('nt8', 'tn8g', 'tn_reduce', 'apply_multi'):
        assert new['kernels'][k]['hbm_bytes_per_launch'] == old['kernels'][k]['hbm_bytes_per_launch']
    # the FETCH_SIZE doubling of the gfx950 note is applied exactly once
    e = new['kernels']['nt8']
    assert e['hbm_bytes_per_launch'] == int(round((2.0 * e['fetch_kib_raw'] + e['write_kib']) * 1024))


def test_bench_json_line_of_the_round_has_the_contract_keys():
    d = json.loads(open(os.path.join(ROOT, 'profiles', 'r03_bench_n1_bf16.json')).read().strip().splitlines()[-1])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['vs_baseline'] is None and d['n_gpus'] == 1 and 'workload' in d['config']
    r = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    c = d['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in c, k
    q = d['qualifying_mode']
    assert q['fresh_max_loss_rel'] <= 1e-4 and q['precision'] in d['modes']


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('bench_module', os.path.join(ROOT, 'bench.py'))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_bench_stdout_line_fits_the_drivers_tail():
    """Round 3's line was 21.5 KB and the driver (8 KB stdout tail) could not parse it: the compact line built from that very
    result must stay under 5 KB, keep the contract keys, and carry roofline / cpu_baseline / parity as scalars."""
    bench = _load_bench()
    full = json.loads(open(os.path.join(ROOT, 'profiles', 'r03_bench_n1_bf16.json')).read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 8192          # (the canned input IS the oversized one)
    full['config']['precision_mode'] = 'bf16: ' + bench.MODE_NOTE['bf16']
    full['throughput_mode'] = {'precision': 'bf16', 'value': 2.0e6, 'unit': 'samples/s', 'ms_per_step': 65.0, 'timed': 'x', 'note': 'y'}
    full['qualifying_mode'] = bench.qualifying_mode(full['modes'])
    line = bench.compact_line(full, 'gpurun_out/bench_detail.json')
    txt = json.dumps(line)
    assert len(txt) < 5000, len(txt)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'parity', 'qualifying_mode', 'throughput_mode'):
        assert k in line, k
    r = line['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in r, k
    assert all(not isinstance(v, (dict, list)) for v in r.values())          # scalars only
    assert set(line['cpu_baseline']) >= {'value', 'unit', 'cores', 'kind', 'sample'}
    assert line['parity']['fresh']['max_loss_rel'] == full['parity']['fresh']['max_loss_rel']
    q = line['qualifying_mode']
    # round 5: a mode qualifies only if it holds the bar in BOTH rollout states of the run: every TERM OF THE LOSS within 1e-4 (the
    # canned run's f16gpx3: stress worst loss term 1.8e-5), kl - no loss term - within 1e-4 fresh / 1e-3 stress (1.76e-4 there)
    assert q['precision'] == 'f16gpx3' and q['fresh_max_loss_rel'] <= 1e-4 and q['stress_ok'] is True
    assert line['parity']['tol']['kl'] == {'fresh_rtol': 1e-4, 'stress_rtol': 1e-3, 'why': line['parity']['tol']['kl']['why']}
    assert line['parity']['tol']['rtol'] == 1e-4 and line['parity']['tol']['atol'] == {'actor_loss': 1e-4, 'enc_loss': 1e-4}
    for k in ('strict_mode', 'fallthrough', 'dist'):
        assert k in line, k
    # every mode name the CLI accepts has its dtype and its one-line description
    assert set(bench.DTYPE_OF) == set(bench.MODE_NOTE) == set(bench.MFMA_PEAK_TFLOPS)


def test_plain_bench_line_keeps_the_contract_keys():
    """A plain run (no --full) has no oracle leg, no roofline pass and no side runs: its line still carries every contract key,
    the headline as given, and null where a --full leg would report."""
    bench = _load_bench()
    full = json.loads(open(os.path.join(ROOT, 'profiles', 'r03_bench_n1_bf16.json')).read().strip().splitlines()[-1])
    extras = ('roofline', 'cpu_baseline', 'parity', 'qualifying_mode', 'throughput_mode', 'strict_mode', 'config5_16384_envs')
    for k in extras:
        full[k] = None
    full['fallthrough'] = []
    line = bench.compact_line(full, None)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data'):
        assert line[k] == full[k], k
    assert all(line[k] is None for k in extras) and line['fallthrough'] == [] and line['detail'] is None
    assert len(json.dumps(line)) < 5000


def test_plain_run_refuses_options_of_the_full_run():
    """--modes and --breakdown only mean something with --full: a plain run stops at the argument check instead of ignoring them."""
    for extra in (['--modes', 'bf16'], ['--breakdown']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and 'need --full' in r.stderr, (extra, r.stderr[-500:])


def test_round4_bench_line_is_compact_and_complete():
    """The driver-form line of round 4 as committed (profiles/r04_bench_n1.json): under the driver's 8 KB tail, headline = the
    qualifying mode, roofline / cpu_baseline / parity present as scalars, fresh-state parity inside BASELINE's 1e-4."""
    raw = open(os.path.join(ROOT, 'profiles', 'r04_bench_n1.json')).read().strip().splitlines()[-1]
    assert len(raw) < 5000
    d = json.loads(raw)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
              'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['scaling'] == 'n/a' and d['vs_baseline'] is None and d['dtype'] == 'f16'
    assert d['config']['precision_mode'].startswith('f16gpx3') and 'workload' in d['config']
    assert abs(d['value'] - d['config']['samples_per_step'] / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    r = d['roofline']
    assert r['bound'] == 'mfma' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and r['traffic'] > r['algorithmic_bytes_per_launch']
    assert set(d['cpu_baseline']) >= {'value', 'unit', 'cores', 'kind', 'sample'} and d['cpu_baseline']['kind'] == 'port'
    p = d['parity']
    assert p['fresh']['ok'] and p['fresh']['max_loss_rel'] <= 1e-4 and p['fresh']['max_count_stat_abs'] <= 1e-3
    assert d['qualifying_mode']['precision'] == 'f16gpx3' and d['qualifying_mode']['is_headline']
    assert d['throughput_mode']['precision'] == 'bf16' and d['throughput_mode']['value'] > d['value']
    assert d['config5_16384_envs']['value'] > 0


def test_round5_bench_line_headline_holds_the_bar():
    """The driver-form line of round 5 as committed (profiles/r05_bench_n1.json): --precision auto chose f16gpx3 with NO fall-through,
    every term of the loss within 1e-4 in both rollout states, the gradient penalty within 1e-5, the tolerances spelled out in the
    line, strict_mode present with a true relative error below 1e-4, and the detail file beside it carries the mask-aware gradients."""
    raw = open(os.path.join(ROOT, 'profiles', 'r05_bench_n1.json')).read().strip().splitlines()[-1]
    assert len(raw) < 5000
    d = json.loads(raw)
    assert d['config']['precision_mode'].startswith('f16gpx3') and d['config']['precision_choice'].startswith('auto')
    assert d['fallthrough'] == [] and d['parity']['headline_ok'] is True
    assert abs(d['value'] - d['config']['samples_per_step'] / (d['ms_per_step'] * 1e-3)) <= 1e-3 * d['value']
    tol = d['parity']['tol']
    assert tol['rtol'] == 1e-4 and tol['atol'] == {'actor_loss': 1e-4, 'enc_loss': 1e-4} and tol['kl'] == {**tol['kl'], 'fresh_rtol': 1e-4, 'stress_rtol': 1e-3}
    for st in ('fresh', 'stress'):
        p = d['parity'][st]
        assert p['ok'] and p['max_loss_term_rel'] <= 1e-4 and p['kl_rel'] <= tol['kl'][st + '_rtol'], (st, p)
        assert p['grad_at_engine_masks']['median_grad_rel_l2'] <= 5e-3
    assert d['parity']['fresh']['grad_at_engine_masks']['worst_grad_rel_l2'] <= 2e-2
    sm = d['strict_mode']
    assert sm['ok'] and sm['fresh_max_true_rel'] <= 1e-4 and sm['stress_max_true_rel'] <= 1e-4 and sm['precision'] in ('bf16x3', 'f32')
    r = d['roofline']
    assert r['bound'] == 'mfma' and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and r['traffic'] > r['algorithmic_bytes_per_launch']
    assert r['traffic_source'] == 'profiles/r05_pmc.json'
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r05_bench_n1_detail.json')))
    for st in ('fresh', 'stress'):
        lr = full['parity'][st]['loss_rel']
        assert lr['disc_grad_penalty'] <= 1e-5, (st, lr['disc_grad_penalty'])


def test_isa_report_parses_a_kernel_and_its_metadata():
    """scripts/isa_report.py on a canned piece of gfx950 assembly: the kernel's resource block, the basic block with the most MFMAs
    and its instruction classes, the kernel-symbol prettifier (binutils' c++filt does not know _Float16's mangling)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('isa_report', os.path.join(ROOT, 'scripts', 'isa_report.py'))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    sym = '_ZN12_GLOBAL__N_115gemm_nt8_kernelIDF16_Lb1ELi256EEEvN6ase_nt8NTParamsE'
    asm = '\n'.join([
        '\t.text', sym + ':', '\ts_load_dwordx4 s[0:3], s[4:5], 0x0', '\tv_mov_b32_e32 v0, 0',
        '.LBB0_1:', '\tds_read_b128 v[2:5], v1', '\tv_mfma_f32_32x32x16_f16 v[10:25], v[2:5], v[6:9], v[10:25]',
        '\tv_mfma_f32_32x32x16_f16 v[10:25], v[2:5], v[6:9], v[10:25]', '\tglobal_load_lds_dwordx4 v[30:31], off', '\ts_barrier',
        '\ts_waitcnt vmcnt(3)', '\ts_setprio 1', '\tv_add_u32_e32 v1, 64, v1', '\ts_cbranch_scc1 .LBB0_1',
        '.LBB0_2:', '\tv_mfma_f32_32x32x16_f16 v[10:25], v[2:5], v[6:9], v[10:25]', '\tglobal_store_dwordx4 v[30:31], v[10:13], off',
        '\ts_endpgm', '\t.amdhsa_kernel ' + sym, '\t.end_amdhsa_kernel',
        'amdhsa.kernels:', '  - .agpr_count:     0', '    .group_segment_fixed_size: 0', '    .max_flat_workgroup_size: 512',
        '    .name:           ' + sym, '    .private_segment_fixed_size: 0', '    .sgpr_count:     77', '    .sgpr_spill_count: 0',
        '    .symbol:         ' + sym + '.kd', '    .vgpr_count:     238', '    .vgpr_spill_count: 0', ''])
    k = {n: v for n, v in R.parse(asm).items() if v['meta']}          # (report() keeps the symbols that own a metadata entry)
    assert list(k) == [sym]
    assert k[sym]['meta']['vgpr_count'] == 238 and k[sym]['meta']['sgpr_count'] == 77 and k[sym]['meta']['max_flat_workgroup_size'] == 512
    assert R.waves_per_simd(k[sym]['meta']) == 2
    best = max(k[sym]['blocks'], key=lambda b: sum(1 for op in b if R.classify(op) == 'mfma'))
    import collections
    c = collections.Counter(R.classify(op) for op in best)
    assert (c['mfma'], c['lds_read'], c['lds_dma'], c['barrier'], c['waitcnt'], c['sched'], c['valu'], c['branch']) == (2, 1, 1, 1, 1, 1, 1, 1)
    assert R.demangle([sym, '_ZN12_GLOBAL__N_114gemm_nt_kernelI6f32h_tLi2ELi2ELi1ELi2ELi128ELi2ELi2ELb0EEEvN6ase_nt8NTParamsE',
                       '_ZN12_GLOBAL__N_116tn_reduce_kernelEPKlPKiPKf']) == \
        ['gemm_nt8_kernel<f16, true, 256>', 'gemm_nt_kernel<f32h_t, 2, 2, 1, 2, 128, 2, 2, false>', 'tn_reduce_kernel']


def test_configure_sets_the_queue_count_once_and_respects_the_user(monkeypatch):
    """ase_amd.configure(): importing the package changes nothing; configure() exports GPU_MAX_HW_QUEUES before HIP
    initialises, leaves a user's value alone, and says what happened in the note the bench line carries."""
    import importlib
    import torch
    import ase_amd
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '1')         # (records the session's own value, restored at teardown)
    monkeypatch.delenv('GPU_MAX_HW_QUEUES')
    # (earlier tests of the same session may have initialised HIP: what configure() does after that is checked below)
    monkeypatch.setattr(torch.cuda, 'is_initialized', lambda: False)
    importlib.reload(ase_amd)
    assert 'GPU_MAX_HW_QUEUES' not in os.environ and not ase_amd.hw_queues_applied and 'not called' in ase_amd.hw_queue_note
    assert ase_amd.configure() is True
    assert os.environ['GPU_MAX_HW_QUEUES'] == ase_amd.HW_QUEUES_DEFAULT == '2' and ase_amd.hw_queues_applied and 'set by ase_amd.configure()' in ase_amd.hw_queue_note
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '1')
    assert ase_amd.configure(hw_queues='2') is True
    assert os.environ['GPU_MAX_HW_QUEUES'] == '1' and 'set by the user' in ase_amd.hw_queue_note
    monkeypatch.delenv('GPU_MAX_HW_QUEUES')
    monkeypatch.setattr(torch.cuda, 'is_initialized', lambda: True)
    assert ase_amd.configure() is False
    assert 'GPU_MAX_HW_QUEUES' not in os.environ and not ase_amd.hw_queues_applied and 'WARNING' in ase_amd.hw_queue_note
    n = torch.get_num_threads()
    ase_amd.configure(cpu_threads=1)
    assert torch.get_num_threads() == 1
    torch.set_num_threads(n)


def test_cfg_tables_follow_the_reference_yaml(golden_dir):
    """ase_amd/cfg: the hyper-parameter tables are the reference's yaml files (their layer widths / activations and scalar
    config entries, as the yaml loader returns them, stored in tests/golden/reference_cfg.json by oracle/make_golden_cfg.py),
    numeric strings of PyYAML ('2e-5') normalised."""
    from ase_amd import cfg as C
    net, conf = C.get('ase')
    assert isinstance(conf['learning_rate'], float) and net['mlp']['units'] == [1024, 1024, 512]
    assert C.normalize({'learning_rate': '2e-5', 'disc_weight_decay': '0.0001'}) == {'learning_rate': 2e-5, 'disc_weight_decay': 1e-4}
    golden = json.load(open(os.path.join(golden_dir, 'reference_cfg.json')))
    assert set(golden) == {'ase', 'amp', 'hrl'}
    for kind in ('ase', 'amp', 'hrl'):
        ref = golden[kind]
        net, conf = C.get(kind)
        for part in ('mlp', 'disc', 'enc'):
            if part in ref['network']:
                assert net[part]['units'] == ref['network'][part]['units'], (kind, part)
                assert net[part]['activation'] == ref['network'][part]['activation'], (kind, part)
        rc = C.normalize(ref['config'])
        for k, v in rc.items():
            if k in conf and isinstance(v, (int, float, bool, str)) and k not in ('name', 'llc_config'):
                assert conf[k] == v, (kind, k, conf[k], v)


def test_bench_dump_outputs_are_float_seeded_and_bounded(tmp_path):
    """bench.py --dump-outputs: the update's per-step results as float64 rows, the weights and normalisers as float32, an array
    above the element cap replaced by a sample whose positions depend on its size only, the whole dump within 64 MB."""
    import types
    import numpy as np
    import torch
    bench = _load_bench()
    model = torch.nn.Module()
    model.register_buffer('running_mean', torch.arange(5, dtype=torch.float64))
    model.register_buffer('count', torch.tensor(3))
    model.a2c_network = types.SimpleNamespace(flat_params=torch.randn(bench.DUMP_MAX_ELEMS + 1000))
    agent = types.SimpleNamespace(model=model)
    info = {'actor_loss': [torch.tensor(1.5), torch.tensor(2.5)], 'last_lr': [2e-5, 2e-5], 'note': ['x', 'y']}
    out = bench.timed_outputs(agent, info)
    assert set(out) == {'update.actor_loss', 'update.last_lr', 'buffer.running_mean', 'params.sample', 'params.sample_index'}
    assert out['update.actor_loss'].dtype == np.float64 and out['update.actor_loss'].tolist() == [1.5, 2.5]
    assert out['buffer.running_mean'].dtype == np.float32 and out['params.sample'].dtype == np.float32
    idx = out['params.sample_index'].astype(np.int64)
    assert len(idx) == bench.DUMP_MAX_ELEMS and np.all(np.diff(idx) > 0)
    assert np.array_equal(out['params.sample'], model.a2c_network.flat_params.numpy()[idx])
    assert np.array_equal(bench.timed_outputs(agent, info)['params.sample_index'], out['params.sample_index'])
    assert sum(a.nbytes for a in out.values()) <= bench.DUMP_BUDGET
    bench.write_outputs(out, str(tmp_path / 'dump'))
    assert sorted(os.listdir(tmp_path / 'dump')) == sorted(k + '.npy' for k in out)
