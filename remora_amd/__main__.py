"""`python -m remora_amd infer from_pod5_and_bam POD5 BAM --model MODEL.pt --out-bam OUT.bam`
— the sub-command of the reference CLI that sits on the hot path (src/remora/parsers.py:1294-1417,
:1582-1612), same positional arguments and the same meaning of --model / --out-bam / --device /
--num-reads; `python -m remora_amd validate from_remora_dataset DATASET --model MODEL.pt` (:1800-1960):
the stored chunks of an on-disk dataset (directory or config) through the model with the model's chunk /
k-mer contexts, the reference's validation summary line against the stored labels; and `python -m remora_amd dataset prepare`
(:64-337), the ETL into the on-disk chunk format, with the bookkeeping verbs around that format (`dataset inspect |
make_config | merge | head | copy`, :359-727: host code over `CoreRemoraDataset` / `RemoraDataset`, no kernel involved);
`python -m remora_amd model train DATASET --model ARCH.py` (:753-1024): ConvLSTM_w_ref in fp32, the training step in HIP;
`model export CHECKPOINT OUT [--format dorado|torchscript]` and `model inspect CHECKPOINT` (:1036-1162): host code, no GPU."""
import argparse
import os
import sys

from . import RemoraError, constants


def _validate(args):
    """src/remora/parsers.py:1890-1960: the dataset is loaded with the model's contexts and without extra arrays,
    every chunk goes through the model, one summary line in the reference's format."""
    import torch

    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset
    from .model_util import load_torchscript_model, winograd_guard_message
    from .validate import ValidationLogger

    from . import dist as rdist

    rank, world, dev = rdist.setup_ranks(args.gpus, args.procs_per_gpu)
    model, md = load_torchscript_model(args.model, device=args.device if dev is None else dev, eval_only=True, dtype=args.dtype)
    if rank == 0 and winograd_guard_message(model, os.path.basename(args.model)):
        print(winograd_guard_message(model, os.path.basename(args.model)), file=sys.stderr)
    over = {"extra_arrays": {}, "kmer_context_bases": md["kmer_context_bases"], "chunk_context": md["chunk_context"]}
    paths, props, hashes = load_dataset(args.remora_dataset_path)
    dataset = RemoraDataset([CoreRemoraDataset(p, override_metadata=dict(over), infinite_iter=False,
                                               do_check_super_batches=True) for p in paths],
                            props, hashes, batch_size=args.batch_size)
    if world > 1:  # this rank's contiguous share of every core dataset's rows
        dataset = dataset.shard(rank, world)
    # rank 0 writes the summary (every rank holds the same global metrics); the per-chunk table is per rank
    sink = open(os.devnull, "w") if rank != 0 else None
    out_fp = sink if sink is not None else (sys.stdout if args.out_file is None else open(args.out_file, "w", buffering=1))
    full_name = args.full_results_filename
    if full_name is not None and world > 1:
        full_name = f"{full_name}.rank{rank:03d}"
    full_fp = None if full_name is None else open(full_name, "w", buffering=1)
    try:
        ValidationLogger(out_fp, full_fp).validate_model(model, md["mod_bases"], torch.nn.CrossEntropyLoss(), dataset,
                                                         args.pct_filt / 100, world=world)
    finally:
        for fp in (out_fp, full_fp):
            if fp not in (None, sys.stdout):
                fp.close()
    rdist.barrier()
    return 0


_IMPLICIT_TAGS = ("If implicit modified tag types (`.`) are included (from all-context modified base models) results from this command "
                  "will be invalid: only the positions an MM tag lists are read, for `.` and `?` alike (what htslib reports; pysam "
                  "issue 1123), so a skipped canonical site of a `.` entry is not counted as a canonical call.")


def _validate_modbams(args):
    """src/remora/parsers.py:1759-1798."""
    import logging

    from .validate import FULL_RESULTS_REFUSAL, validate_modbams

    log = logging.getLogger("Remora")
    log.setLevel(logging.INFO)
    log.addHandler(logging.StreamHandler(sys.stderr))
    if args.explicit_mod_tag_used:
        log.warning(_IMPLICIT_TAGS)
    else:
        log.error(_IMPLICIT_TAGS + " To force the usage of this command please specify the --explicit-mod-tag-used argument")
        return 1
    if args.full_results_filename is not None:
        raise RemoraError(FULL_RESULTS_REFUSAL)
    if args.log_filename is not None:
        log.addHandler(logging.FileHandler(args.log_filename, mode="w"))
    line = validate_modbams(bams_and_beds=args.bam_and_bed, full_results_path=None, name=args.name, pct_filt=args.pct_filt,
                            allow_unbalanced=args.allow_unbalanced, seed=args.seed, extra_bases=args.extra_bases,
                            max_sites_per_read=args.max_sites_per_read, device=args.device)
    sys.stdout.write(line.lstrip("\n"))
    log.info("Done")
    return 0


def _dataset_prepare(args):
    """src/remora/parsers.py:281-337."""
    from .engine import get_engine
    from .io import parse_bed
    from .prepare_train_data import extract_chunk_dataset
    from .refine_signal_map import SigMapRefiner
    from .util import Motif, prepare_out_dir

    if args.mod_base is None and not args.mod_base_control:
        raise RemoraError("Must specify either --mod-base or --mod-base-control")
    from . import dist as rdist

    rank, world, dev = rdist.setup_ranks(args.gpus, args.procs_per_gpu)
    if rank == 0:
        prepare_out_dir(args.output_path, args.overwrite)
    rdist.barrier()
    refiner = SigMapRefiner(kmer_model_filename=args.refine_kmer_level_table, do_rough_rescale=args.refine_rough_rescale,
                            scale_iters=args.refine_scale_iters, algo=args.refine_algo,
                            half_bandwidth=args.refine_half_bandwidth, sd_params=args.refine_short_dwell_parameters,
                            do_fix_guage=True, rough_rescale_method=args.rough_rescale_method)
    if not refiner.is_valid:
        raise RemoraError("Invalid signal mapping refiner settings.")
    dataset, errs = extract_chunk_dataset(
        bam_path=args.bam, pod5_path=args.pod5, out_path=args.output_path, mod_base=args.mod_base,
        mod_base_control=args.mod_base_control, motifs=[Motif(*m) for m in args.motif],
        focus_ref_pos=None if args.focus_reference_positions is None else parse_bed(args.focus_reference_positions),
        chunk_context=args.chunk_context, min_samps_per_base=args.min_samples_per_base,
        max_chunks_per_read=args.max_chunks_per_read, pa_scaling=None, sig_map_refiner=refiner,
        kmer_context_bases=args.kmer_context_bases, base_start_justify=args.base_start_justify, offset=args.offset,
        num_reads=args.num_reads, basecall_anchor=args.basecall_anchor, rev_sig=args.reverse_signal,
        save_every=args.save_every, skip_shuffle=args.skip_shuffle, reads_per_batch=args.reads_per_batch,
        engine=get_engine(args.device if dev is None else dev), rank=rank, world=world)
    if rank != 0:
        return 0
    if dataset is None:
        print("no reads with signal and alignment")
        return 0
    for reason, cnt in sorted(errs.items(), key=lambda kv: -kv[1]):
        print(f"{cnt:>7,} : {reason}")
    print(f"Extracted {dataset.size:,} chunks -> {args.output_path}")
    print(f"Label distribution: {dataset.label_summary}")
    return 0


def _dataset_inspect(args):
    """src/remora/parsers.py:359-376."""
    import json

    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset

    paths, props, hashes = load_dataset(args.remora_dataset_path)
    dataset = RemoraDataset([CoreRemoraDataset(p, do_check_super_batches=True) for p in paths], props, hashes)
    print(f"Dataset summary:\n{dataset.summary}")
    if args.out_path is not None:
        with open(args.out_path, "w") as fh:
            json.dump(dataset.get_config(), fh)
    return 0


def _dataset_make_config(args):
    """src/remora/parsers.py:414-458: default weights are the dataset sizes (chunks drawn uniformly overall)."""
    import json

    import numpy as np

    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset

    if args.dataset_weights is not None:
        if len(args.dataset_weights) != len(args.dataset_paths):
            raise RemoraError("Weights must be same length as input datasets.")
        if any(w <= 0 for w in args.dataset_weights):
            raise RemoraError("Weights must be positive.")
    core_paths, core_weights, core_hashes = [], [], []
    for i, ds_path in enumerate(args.dataset_paths):
        paths, weights, hashes = load_dataset(ds_path)
        core_paths.extend(paths)
        scale = sum(CoreRemoraDataset(p).size for p in paths) if args.dataset_weights is None else args.dataset_weights[i]
        core_weights.extend(weights * scale)
        if hashes is None or core_hashes is None:
            core_hashes = None
        else:
            core_hashes.extend(hashes)
    core_weights = np.array(core_weights)
    dataset = RemoraDataset([CoreRemoraDataset(p) for p in core_paths], core_weights / core_weights.sum(), core_hashes)
    with open(args.out_path, "w") as fh:
        json.dump(dataset.get_config(), fh)
    print(dataset.summary)
    return 0


def _dataset_merge(args):
    """src/remora/parsers.py:493-572: all rows of several datasets (labels converted to the merged label set)
    copied into one new dataset, optionally capped at --max-size in proportion, then shuffled."""
    import numpy as np

    from .data_chunks import CoreRemoraDataset, RemoraDataset, compute_best_split, load_dataset
    from .util import prepare_out_dir

    prepare_out_dir(args.out_path, args.overwrite)
    paths = [sub for ds_path in args.dataset_paths for sub in load_dataset(ds_path)[0]]
    dataset = RemoraDataset([CoreRemoraDataset(p, infinite_iter=False, do_check_super_batches=True) for p in paths],
                            np.ones(len(paths)) / len(paths))
    sizes = np.array([ds.size for ds in dataset.datasets])
    if args.max_size is not None and sizes.sum() > args.max_size:
        sizes = compute_best_split(args.max_size, sizes / sizes.sum())
    md = dataset.metadata.copy()
    md.allocate_size, md.max_seq_len = int(sizes.sum()), max(ds.metadata.max_seq_len for ds in dataset.datasets)
    md.dataset_start = md.dataset_end = 0
    merged = CoreRemoraDataset(data_path=args.out_path, mode="w", metadata=md)
    for ds, size in zip(dataset.datasets, sizes):
        ds.metadata.dataset_end = ds.metadata.dataset_start + int(size)
        ds.adjust_batch_params()
        for sb in ds.iter_super_batches():
            merged.write_batch(sb)
        merged.flush()
    merged.shuffle()
    merged.flush()
    print(f"Saved core dataset:\n{merged.summary}")
    return 0


def _dataset_head(args):
    """src/remora/parsers.py:604-655: the first `num_chunks` rows of a core dataset as a new (shuffled) dataset."""
    from .data_chunks import CoreRemoraDataset
    from .util import prepare_out_dir

    prepare_out_dir(args.out_path, args.overwrite)
    src = CoreRemoraDataset(args.in_path, infinite_iter=False, do_check_super_batches=True)
    md = src.metadata.copy()
    md.allocate_size, md.dataset_start, md.dataset_end = args.num_chunks, 0, 0
    head = CoreRemoraDataset(data_path=args.out_path, mode="w", metadata=md)
    src.adjust_batch_params()
    for sb in src.iter_super_batches():
        room = args.num_chunks - head.metadata.dataset_end
        if sb["labels"].size >= room:
            head.write_batch({n: a[:room] for n, a in sb.items()})
            break
        head.write_batch(sb)
    head.flush()
    head.shuffle()
    head.flush()
    print(f"Saved core dataset:\n{head.summary}")
    return 0


def _dataset_copy(args):
    """src/remora/parsers.py:684-727: every core dataset of a dataset / config copied to OUT/dataset_NNN, with
    OUT/dataset.cfg pointing at the copies and OUT/sources.txt recording where they came from."""
    import json
    import os
    import shutil

    from .data_chunks import CoreRemoraDataset, RemoraDataset, load_dataset
    from .util import prepare_out_dir

    prepare_out_dir(args.out_path, args.overwrite)
    paths, props, hashes = load_dataset(args.in_path)
    out_dirs = []
    with open(os.path.join(args.out_path, "sources.txt"), "w") as src_fh:
        for i, src in enumerate(paths):
            if any(os.path.isdir(os.path.join(src, item)) for item in os.listdir(src)):
                raise RemoraError(f"Source dataset has nested directory: {src}")
            dst = os.path.join(args.out_path, f"dataset_{i:03}")
            src_fh.write(f"{src}\t{dst}\n")
            shutil.copytree(src, dst)
            out_dirs.append(dst)
    dataset = RemoraDataset([CoreRemoraDataset(d) for d in out_dirs], props, hashes)
    with open(os.path.join(args.out_path, "dataset.cfg"), "w") as fh:
        json.dump(dataset.get_config(), fh)
    print(dataset.summary)
    return 0


def _infer(args):
    from . import dist as rdist
    from .inference import infer_from_pod5_and_bam
    from .model_util import load_torchscript_model, winograd_guard_message

    # this rank's share of the BAM, found in a thread under the model load.  By byte range (default): where the share and
    # the next one begin is read off the bytes there (io.bam_byte_shard - no pass over the file, and the rank in front
    # verifies the guess); REMORA_AMD_BAM_SHARD=scan: by record count from one exact pass (the launcher's, or this rank's own)
    erank, eworld, _ = rdist.env_rank_world()
    shard_future = None
    if eworld > 1:
        from concurrent.futures import ThreadPoolExecutor

        from . import io as rio

        shard_future = ThreadPoolExecutor(max_workers=1).submit(rio.shard_of, args.in_bam, erank, eworld)
    rank, world, dev = rdist.setup_ranks(args.gpus, args.procs_per_gpu)
    loaded = [load_torchscript_model(m, device=args.device if dev is None else dev, eval_only=True, dtype=args.dtype)
              for m in args.model]
    model, md = [x[0] for x in loaded], [x[1] for x in loaded]
    for name, mdl in zip(args.model, model):
        if rank == 0 and winograd_guard_message(mdl, os.path.basename(name)):
            print(winograd_guard_message(mdl, os.path.basename(name)), file=sys.stderr)
    if len({m["can_base"] for m in md}) != len(md):
        raise RemoraError("Only one model per canonical base allowed.")
    import time

    label_counts = {}
    rdist.barrier()  # every rank has its model: the clock below covers the file-to-file work, not interpreter start-up
    t0 = time.perf_counter()
    stats = infer_from_pod5_and_bam(args.pod5, args.in_bam, model, md, args.out_bam, num_reads=args.num_reads,
                                    reads_per_batch=args.reads_per_batch, ref_anchored=args.reference_anchored,
                                    rank=rank, world=world, label_counts_out=label_counts, bam_level=args.bam_level,
                                    shard_future=shard_future)
    dt = time.perf_counter() - t0
    if rank != 0:
        return 0
    ok = stats.pop(None, 0)
    nrec = ok + sum(stats.values())
    print(f"{nrec} records in {dt:.2f} s = {nrec / max(dt, 1e-9):.0f} reads/s (models loaded; parts joined)", file=sys.stderr)
    print(f"called {ok} reads -> {args.out_bam}" + (f" ({args.gpus} GPUs" + (f" x {args.procs_per_gpu} processes" if args.procs_per_gpu > 1 else "") + ")"
                                                  if world > 1 else ""))
    for reason, cnt in sorted(stats.items(), key=lambda kv: -kv[1]):
        print(f"{cnt:>7} : {reason}")
    for m in md:
        names = ["canonical"] + list(m["mod_long_names"])
        print(f"calls per label ({m['can_base']}): " + "; ".join(f"{n}:{int(c)}" for n, c in zip(names, label_counts[m["can_base"]])))
    return 0


def _infer_duplex(args):
    """src/remora/parsers.py:1615-1662."""
    import logging

    from .inference import infer_duplex
    from .model_util import load_torchscript_model

    log = logging.getLogger("Remora")
    log.setLevel(logging.INFO)
    if not log.handlers:
        log.addHandler(logging.StreamHandler(sys.stderr))
    if args.log_filename is not None:
        log.addHandler(logging.FileHandler(args.log_filename, mode="w"))
    if len(args.model) > 1:  # refused before anything is loaded
        raise NotImplementedError("Duplex infer does not currently implement running of multiple models")
    for what, path in (("pod5", args.pod5), ("simplex bam", args.simplex_bam), ("duplex bam", args.duplex_bam),
                       ("duplex read pairs", args.duplex_read_pairs)):
        if not os.path.exists(path):
            raise ValueError(f"didn't find {what} at {path}")
    model, md = load_torchscript_model(args.model[0], device=args.device, eval_only=True, dtype=args.dtype)
    infer_duplex(simplex_pod5_path=args.pod5, simplex_bam_path=args.simplex_bam, duplex_bam_path=args.duplex_bam,
                 pairs_path=args.duplex_read_pairs, model=model, model_metadata=md, out_bam=args.out_bam,
                 num_extract_alignment_threads=args.num_extract_alignment_workers, num_duplex_prep_workers=args.num_duplex_prep_workers,
                 num_infer_threads=args.num_infer_workers, num_reads=args.num_reads, duplex_deliminator=args.duplex_delim,
                 reads_per_batch=args.reads_per_batch, bam_level=args.bam_level, trace_budget=int(args.duplex_trace_gib * (1 << 30)))
    log.info("Done")
    return 0


def _estimate_kmer_levels(args):
    """src/remora/parsers.py:2268-2333."""
    import logging

    import numpy as np

    from .engine import get_engine
    from .io import read_bam_header_bytes, run_site_level_ranges
    from .metrics import LEVEL_BYTES_PER_BASE, SiteLevels, kmer_strings
    from .refine_signal_map import SigMapRefiner

    log = logging.getLogger("Remora")
    if args.log_filename is not None:
        log.addHandler(logging.FileHandler(args.log_filename, mode="w"))
        log.setLevel(logging.INFO)
    out_fh = open(args.levels_filename, "w")  # opened first: no long run without write access
    refiner = SigMapRefiner(kmer_model_filename=args.refine_kmer_level_table, do_rough_rescale=args.refine_rough_rescale,
                            scale_iters=args.refine_scale_iters, algo=args.refine_algo, half_bandwidth=args.refine_half_bandwidth,
                            sd_params=args.refine_short_dwell_parameters, do_fix_guage=True)
    if not refiner.is_loaded or refiner.scale_iters < 0:
        log.warning("It is highly recommended to apply signal mapping refinement in order to output a valid kmer level table.")
    log.info("--chunk-width, --max-chunk-coverage and --num-workers are ignored: the BAM is streamed once and every read is used")
    import torch

    eng = get_engine(args.device)
    if not args.levels_device_gib > 0:
        raise RemoraError("--levels-device-gib must be positive")
    free = torch.cuda.mem_get_info(eng.torch_device)[0]
    gib = min(float(args.levels_device_gib), free / 2 / 2**30)
    max_resident = int(gib * 2**30 // LEVEL_BYTES_PER_BASE)
    log.info(f"k-mer levels aggregate in {gib:.3g} GiB of device memory ({max_resident} bases at a time; --levels-device-gib "
             f"{args.levels_device_gib:g}, {free / 2**30:.1f} GiB free)")
    acc = SiteLevels(eng, args.kmer_context_bases, args.min_coverage, max_resident)
    pairs = []
    for sample, (pod5_path, bam_path) in enumerate(args.pod5_and_bam):
        hdr = read_bam_header_bytes(bam_path)
        l_text = int.from_bytes(hdr[4:8], "little")
        if int.from_bytes(hdr[8 + l_text : 12 + l_text], "little") == 0:
            log.warning("Cannot estimate levels from BAM file without mappings or index")
            continue
        log.info(f"Extracting levels from {pod5_path} and {bam_path}")
        pairs.append((sample, pod5_path, bam_path))
    n_ranges, _ = run_site_level_ranges(acc, pairs, refiner, reads_per_batch=args.reads_per_batch, device=args.device,
                                        reverse_signal=args.reverse_signal, log=log.info)
    log.info(f"Aggregated in {n_ranges} ranges")
    log.info("Aggregating and outputting levels")
    levels, _ = acc.levels()
    if np.isnan(levels).any():
        log.warning("Some k-mers not observed.")
    for kmer, level in zip(kmer_strings(acc.kmer_len), levels.tolist()):
        out_fh.write(f"{kmer}\tnan\n" if level != level else f"{kmer}\t{np.float64(level)}\n")
    out_fh.close()
    log.info("Done")
    return 0


def _partition_tag(text):
    """argparse type of --partition-tag: the refusal of a malformed tag name as the parser's error."""
    import argparse

    from .pileup import check_partition_tag

    try:
        return check_partition_tag(text)
    except RemoraError as e:
        raise argparse.ArgumentTypeError(str(e))


def _pileup_modbams(args):
    """`analyze pileup_modbams` (no counterpart in the reference's command line): per-site modified-base counts, bedMethyl."""
    import logging

    from .pileup import (check_hemi_arguments, check_ref_arguments, partition_file_name, pileup_modbams, write_bedmethyl, write_counts,
                         write_partitioned)

    if args.coverage_columns and (args.duplex or args.hemi):  # before any file is opened or written, the log included
        raise RemoraError(f"--coverage-columns with {'--hemi' if args.hemi else '--duplex'} is not built: there a record stands for two "
                          "strands; give one of them")
    log = logging.getLogger("Remora")
    log.setLevel(logging.INFO)
    if not log.handlers:
        log.addHandler(logging.StreamHandler(sys.stderr))
    if args.log_filename is not None:
        log.addHandler(logging.FileHandler(args.log_filename, mode="w"))
    if args.min_coverage < 1:
        raise RemoraError("--min-coverage is at least 1")
    motifs = check_ref_arguments(args.ref, args.motif, args.cpg, args.combine_strands, args.canonical_base)
    if args.hemi:
        check_hemi_arguments(args.ref, motifs, args.combine_strands, args.partition_tag, [args.canonical_base] + list(args.mod_bases))
    table = pileup_modbams(args.bam, [args.canonical_base] + list(args.mod_bases), filter_threshold=args.filter_threshold,
                           pct_filt=args.pct_filt, region=args.region, device=args.device, batch=args.reads_per_batch,
                           device_gib=args.pileup_device_gib, ref=args.ref, motifs=motifs, combine_strands=args.combine_strands,
                           partition_tag=args.partition_tag, duplex=args.duplex, hemi=args.hemi, coverage=args.coverage_columns)
    # the files are written only now: a run that keeps no call leaves none behind
    if args.partition_tag is not None:  # --out-bed and --counts-filename are templates: one file per partition that has a row
        rows = write_partitioned(table, args.out_bed, args.counts_filename, min_coverage=args.min_coverage)
        log.info(f"bedMethyl rows per {args.partition_tag}: " + ", ".join(f"{label}: {n}" for label, n in rows.items()) +
                 f" ({table.pos.size} rows of partition and site) -> " +
                 ", ".join(partition_file_name(args.out_bed, args.partition_tag, label) for label in rows))
        log.info("Done")
        return 0
    n_rows = write_bedmethyl(table, args.out_bed, min_coverage=args.min_coverage)
    if args.counts_filename is not None:
        write_counts(table, args.counts_filename)
    log.info(f"{n_rows} bedMethyl rows of {table.pos.size} sites -> {args.out_bed}")
    log.info("Done")
    return 0


def _model_train(args):
    """src/remora/parsers.py:977-1024."""
    import logging

    from .model_util import TrainOpts
    from .train_model import train_model
    from .util import prepare_out_dir

    log = logging.getLogger("Remora")
    log.setLevel(logging.INFO)
    if not log.handlers:
        log.addHandler(logging.StreamHandler(sys.stderr))
    # what is refused is refused before the output directory is touched
    if args.optimizer != "AdamW":
        raise RemoraError(f"--optimizer {args.optimizer}: the HIP trainer implements AdamW only")
    if args.finetune_path is not None or args.freeze_num_layers:
        raise RemoraError("--finetune-path / --freeze-num-layers: fine-tuning is not built for the HIP trainer")
    from .model_util import scan_model_file

    if scan_model_file(args.model) != "conv_lstm":
        raise RemoraError(f"--model {args.model} assigns the layers of Conv_w_ref: the HIP trainer trains ConvLSTM_w_ref only")
    device = args.device
    if device is not None:
        device = int(device) if str(device).isdigit() else device
    # argparse appends to the default list in the reference: what is given is added to (and overrides) the defaults
    opt_kwargs = list(constants.DEFAULT_OPT_VALUES) + [tuple(x) for x in (args.optimizer_kwargs or [])]
    sch_kwargs = list(constants.DEFAULT_SCH_VALUES) + [tuple(x) for x in (args.lr_scheduler_kwargs or [])]
    prepare_out_dir(args.output_path, args.overwrite)
    train_opts = TrainOpts(epochs=args.epochs, early_stopping=args.early_stopping, optimizer_str=args.optimizer,
                           opt_kwargs=opt_kwargs, learning_rate=args.lr, lr_scheduler_str=args.lr_scheduler,
                           lr_scheduler_kwargs=sch_kwargs, lr_cool_down_epochs=args.lr_cool_down_epochs,
                           lr_cool_down_lr=args.lr_cool_down_learning_rate)
    train_model(args.seed, device, args.output_path, args.remora_dataset_path, args.chunk_context, args.kmer_context_bases,
                args.batch_size, args.model, args.size, train_opts, args.chunks_per_epoch, args.num_test_chunks, args.save_freq,
                args.filter_fraction, args.ext_val, args.ext_val_names, args.high_conf_incorrect_thr_frac, args.finetune_path,
                args.freeze_num_layers, args.super_batch_size, args.super_batch_sample_fraction, args.read_batches_from_disk,
                args.gradient_clip_num_mads)
    log.info("Done")
    return 0


def _load_for_export(args, log):
    """(checkpoint-like dict, state, came from a checkpoint) of `model export` / `model inspect`: the input as a TorchScript
    model first (its metadata as load_model returns it, without an engine), failing that as a training checkpoint
    (src/remora/parsers.py:1063-1070)."""
    from .model_util import _raw_load_torchscript_model, add_derived_metadata, load_checkpoint

    log.info("Loading model")
    try:
        if not os.path.isfile(args.checkpoint_path):
            raise RuntimeError("not a file")
        state, md = _raw_load_torchscript_model(args.checkpoint_path)
    except RuntimeError:  # what torch.jit.load says to a file that is no TorchScript archive
        ckpt = load_checkpoint(args.checkpoint_path, args.model_path)
        log.info("Loaded model from checkpoint")
        return ckpt, ckpt["state_dict"], True
    add_derived_metadata(md)
    if args.model_path is not None:
        from .engine import detect_arch
        from .model_util import scan_model_file

        arch, scanned = detect_arch({k.split(".")[0] for k in state}), scan_model_file(args.model_path)
        if scanned != arch:
            raise RemoraError(f"--model-path {args.model_path} assigns the layers of a {scanned} network, the model's state is "
                              f"that of a {arch} network")
    log.info("Loaded a torchscript model")
    return md, state, False


def _model_log():
    import logging

    log = logging.getLogger("Remora")
    log.setLevel(logging.INFO)
    if not log.handlers:
        log.addHandler(logging.StreamHandler(sys.stderr))
    return log


def _model_inspect(args):
    """src/remora/parsers.py:1055-1104.  No engine, no GPU."""
    from .model_util import refiner_from_checkpoint, repr_model_metadata

    log = _model_log()
    md, _, from_ckpt = _load_for_export(args, log)
    if from_ckpt:
        md = dict(md)
        md["sig_map_refiner"] = refiner_from_checkpoint(md)
        if md.get("refine_kmer_levels") is None:  # models from before the refiner
            md["base_start_justify"], md["offset"] = False, 0
        for key in [k for k in md if k.startswith("refine_")] + ["state_dict", "opt"]:
            md.pop(key, None)
    log.info(f"Loaded Remora model attrs\n{repr_model_metadata(md)}\n")
    log.info("Done")
    return 0


def _model_export(args):
    """src/remora/parsers.py:1136-1162.  No engine, no GPU."""
    from .model_util import export_model_dorado, export_model_torchscript

    log = _model_log()
    ckpt, state, from_ckpt = _load_for_export(args, log)
    if args.format == "dorado":
        log.info("Exporting model to dorado format")
        export_model_dorado(ckpt, state, args.output_path)
    else:
        log.info("Exporting model to TorchScript format")
        if not from_ckpt:  # the refiner's entries, which add_derived_metadata folded into sig_map_refiner
            ckpt = {**ckpt["sig_map_refiner"].asdict(), **ckpt}
        export_model_torchscript(ckpt, state, args.output_path)
    log.info("Done")
    return 0


def _add_model_export_inspect(model):
    """The reference's arguments (src/remora/parsers.py:1036-1052, :1107-1133)."""
    e = model.add_parser("export", help="Export a trained model for deployment: a dorado-format directory or a TorchScript file")
    e.add_argument("checkpoint_path", help="a training checkpoint, or a TorchScript model file")
    e.add_argument("output_path", help="directory (dorado) or file (torchscript) to save the model to")
    e.add_argument("--model-path", help="model architecture file: scanned for its layer names, never executed (default: the checkpoint's)")
    e.add_argument("--format", default="dorado", choices=["dorado", "torchscript"], help="export format")
    e.set_defaults(func=_model_export)
    i = model.add_parser("inspect", help="Print the attributes of a training checkpoint or a TorchScript model file")
    i.add_argument("checkpoint_path", help="a training checkpoint, or a TorchScript model file")
    i.add_argument("--model-path", help="model architecture file: scanned for its layer names, never executed (default: the checkpoint's)")
    i.set_defaults(func=_model_inspect)


def _add_model_train(model):
    """The reference's arguments (src/remora/parsers.py:753-975)."""
    t = model.add_parser(
        "train", help="Train a ConvLSTM_w_ref model on an MI355X (fp32; forward, backward and AdamW in HIP)")
    t.add_argument("remora_dataset_path", help="Remora training dataset (directory or config)")
    g = t.add_argument_group("Data Arguments")
    g.add_argument("--batch-size", default=constants.DEFAULT_BATCH_SIZE, type=int)
    g.add_argument("--chunk-context", type=int, nargs=2, metavar=("NUM_BEFORE", "NUM_AFTER"), help="override the chunk context of data prep")
    g.add_argument("--kmer-context-bases", type=int, nargs=2, metavar=("BASES_BEFORE", "BASES_AFTER"),
                   help="override the k-mer context bases of data prep")
    g.add_argument("--ext-val", nargs="+", help="external validation datasets")
    g.add_argument("--ext-val-names", nargs="+", help="names of the external datasets (as many as --ext-val)")
    g.add_argument("--chunks-per-epoch", default=constants.DEFAULT_CHUNKS_PER_EPOCH, type=int)
    g.add_argument("--num-test-chunks", default=constants.DEFAULT_NUM_TEST_CHUNKS, type=int)
    g.add_argument("--filter-fraction", default=constants.DEFAULT_FILT_FRAC, type=float)
    g.add_argument("--read-batches-from-disk", action="store_true", help="accepted and ignored: validation batches are always read from disk")
    g = t.add_argument_group("Output Arguments")
    g.add_argument("--output-path", default="remora_train_results")
    g.add_argument("--save-freq", default=10, type=int, help="save the model every this many epochs")
    g.add_argument("--overwrite", action="store_true")
    g = t.add_argument_group("Model Arguments")
    g.add_argument("--model", required=True, help="model architecture file: copied to the output, scanned for its layer names, never executed")
    g.add_argument("--finetune-path", help="refused: fine-tuning is not built")
    g.add_argument("--freeze-num-layers", default=0, type=int, help="refused unless 0")
    g.add_argument("--size", type=int, default=constants.DEFAULT_NN_SIZE, help="layer size: a multiple of 16 from 16 to 256")
    g = t.add_argument_group("Training Arguments")
    g.add_argument("--epochs", default=constants.DEFAULT_EPOCHS, type=int)
    g.add_argument("--optimizer", default=constants.DEFAULT_OPTIMIZER, help="AdamW (anything else is refused)")
    g.add_argument("--optimizer-kwargs", nargs=3, action="append", default=None, metavar=("NAME", "VALUE", "TYPE"),
                   help="lr / weight_decay / eps of AdamW; TYPE is str, int or float (default: weight_decay 1e-4 float)")
    g.add_argument("--lr", default=constants.DEFAULT_LR, type=float,
                   help="as in the reference this value does not reach the optimiser: give `--optimizer-kwargs lr VALUE float`")
    g.add_argument("--lr-scheduler", default=constants.DEFAULT_SCHEDULER, help="a torch.optim.lr_scheduler class")
    g.add_argument("--lr-scheduler-kwargs", nargs=3, action="append", default=None, metavar=("NAME", "VALUE", "TYPE"))
    g.add_argument("--lr-cool-down-epochs", type=int, default=constants.DEFAULT_SCH_COOL_DOWN_EPOCHS)
    g.add_argument("--lr-cool-down-learning-rate", type=float, default=constants.DEFAULT_SCH_COOL_DOWN_LR)
    g.add_argument("--early-stopping", default=constants.DEFAULT_EARLY_STOPPING, type=int, help="0: never stop early")
    g.add_argument("--seed", type=int)
    g.add_argument("--high-conf-incorrect-thr-frac", nargs=2, type=float, metavar=("THRESHOLD", "FRACTION"),
                   help="leave confidently wrong chunks out of each iteration's loss (they still take part in BatchNorm)")
    g.add_argument("--gradient-clip-num-mads", default=0, type=lambda x: None if x == "None" else float(x),
                   help="clip gradients by value at this many MADs above the median of the last 1000 maxima; None: no clipping")
    g = t.add_argument_group("Compute Arguments")
    g.add_argument("--device", default=None, help="GPU index or torch device string")
    g.add_argument("--super-batch-size", default=constants.DEFAULT_SUPER_BATCH_SIZE, type=int)
    g.add_argument("--super-batch-sample-fraction", default=constants.DEFAULT_SUPER_BATCH_SAMPLE_FRAC, type=float)
    t.set_defaults(func=_model_train)


POD5_HELP = ("POD5 file, or a run's directory of POD5 files: the files named *.pod5 directly in it (sub-directories are not walked), "
             "in sorted order; a read id that several files hold is taken from the first and the repeats are counted in one warning.  "
             "The ids of a directory are an index on the GPU; every process (--gpus / --procs-per-gpu rank) builds its own")


def build_parser():
    ap = argparse.ArgumentParser(prog="remora_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    model = sub.add_parser("model").add_subparsers(dest="sub", required=True)
    _add_model_train(model)
    _add_model_export_inspect(model)
    infer = sub.add_parser("infer").add_subparsers(dest="sub", required=True)
    p = infer.add_parser("from_pod5_and_bam", help="Infer modified bases from POD5 + BAM on an MI355X")
    p.add_argument("pod5", help=POD5_HELP)
    p.add_argument("in_bam")
    p.add_argument("--model", required=True, action="append",
                   help="TorchScript model file (with meta.txt) or dorado-format model directory; repeat for one model per canonical base")
    p.add_argument("--out-bam", required=True)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--gpus", type=int, default=1,
                   help="one process per GPU, each takes a contiguous share of the alignments (ranks are started here unless "
                        "already under torchrun); the parts are joined into --out-bam in input order")
    p.add_argument("--procs-per-gpu", type=int, default=1,
                   help="processes per GPU: the host side (BAM / POD5 parsing, per-read arithmetic, MM/ML formatting, BGZF) is "
                        "Python and scales with processes; each takes its own contiguous share of the alignments (and, for a "
                        "directory of POD5 files, builds its own read-id index)")
    p.add_argument("--bam-level", type=int, default=None, help="zlib level of the output BAM (default 6, as htslib; 1 = fast: Huffman coding only, about a fifth larger, half the CPU time of zlib's level 1)")
    p.add_argument("--num-reads", type=int, default=None)
    p.add_argument("--reads-per-batch", type=int, default=512)
    p.add_argument("--dtype", default=None, help="fp32 (default) | f16x3 (fp32-class accuracy inside IEEE half's range: inputs and folded weights beyond +-65504 overflow) | "
                        "bf16x6 (fp32 class, fp32 range) | bf16x3 | bf16 | f16")
    p.add_argument("--reference-anchored", action="store_true",
                   help="call at reference positions; output records become <len>M with the reference sequence")
    p.set_defaults(func=_infer)

    d = infer.add_parser("duplex_from_pod5_and_bam", help="Infer modified bases on duplex reads from POD5 + simplex BAM + duplex BAM "
                                                          "with duplex pairs (src/remora/parsers.py:1420-1535)")
    d.add_argument("pod5", help="matched to the simplex BAM: " + POD5_HELP)
    d.add_argument("simplex_bam", help="basecalled BAM file containing mv tags")
    d.add_argument("duplex_bam", help="BAM file with the duplex basecalls; record names are the template read id or "
                                      "template<delim>complement")
    d.add_argument("duplex_read_pairs", help="whitespace separated text file of template / complement read id pairs, no header")
    d.add_argument("--duplex-delim", default=";", help="string between the template and complement read ids in the duplex BAM")
    d.add_argument("--out-bam", required=True)
    d.add_argument("--log-filename")
    d.add_argument("--model", required=True, action="append", help="TorchScript model file (with meta.txt) or dorado-format model directory; one model only")
    d.add_argument("--num-reads", type=int, default=None, help="number of (valid) pairs")
    d.add_argument("--device", type=int, default=0)
    for flag in ("--num-extract-alignment-workers", "--num-duplex-prep-workers", "--num-infer-workers"):
        d.add_argument(flag, type=int, default=1, help="accepted and ignored: the pairs go through the GPU in batches")
    d.add_argument("--dtype", default=None, help="as for infer from_pod5_and_bam")
    d.add_argument("--bam-level", type=int, default=None, help="as for infer from_pod5_and_bam")
    d.add_argument("--reads-per-batch", type=int, default=64, help="duplex pairs per batch: two alignments and two model passes each")
    d.add_argument("--duplex-trace-gib", type=float, default=16.0,
                   help="GiB of GPU memory the simplex-to-duplex alignments of a batch may take at a time; a batch that does not fit "
                        "with whole traces runs in checkpointed memory (same alignments, any read length)")
    d.set_defaults(func=_infer_duplex)

    val = sub.add_parser("validate").add_subparsers(dest="sub", required=True)
    v = val.add_parser("from_remora_dataset", help="Validate a model on an on-disk Remora dataset (directory or config)")
    v.add_argument("remora_dataset_path")
    v.add_argument("--model", required=True, help="TorchScript model file (with meta.txt) or dorado-format model directory")
    v.add_argument("--out-file", help="validation summary (default stdout)")
    v.add_argument("--full-results-filename", help="per-chunk label, call and probabilities (TSV)")
    v.add_argument("--pct-filt", type=float, default=10.0)
    v.add_argument("--device", type=int, default=0)
    v.add_argument("--gpus", type=int, default=1,
                   help="one process per GPU, each validates a contiguous share of the rows; confusion counts are all-reduced")
    v.add_argument("--procs-per-gpu", type=int, default=1)
    v.add_argument("--batch-size", type=int, default=131072)
    v.add_argument("--dtype", default=None)
    v.set_defaults(func=_validate)

    vm = val.add_parser("from_modbams", help="Validation with ground truth samples: the MM/ML calls of mapped BAM files scored at "
                        "the sites of ground-truth BED files (tags tokenised on native threads, calls, alignment and sites joined on the GPU)")
    vm.add_argument("--bam-and-bed", required=True, nargs=2, metavar=("BAM", "GROUND_TRUTH_BED"), action="append",
                    help="BAM file with modified base tags (mapped, with MD tags) and a BED file with ground truth reference positions, "
                         "whose name field is the single letter code of a modified base or of the canonical base; repeat for several samples")
    vm.add_argument("--full-results-filename", help="the reference's per-pair alignment-context TSV: not built here, refused")
    vm.add_argument("--name", default="sample", help="Name of this sample/comparison. Useful when tabulating several runs.")
    vm.add_argument("--pct-filt", type=float, default=10.0, help="Filter a specified percentage (or less given ties) of calls.")
    vm.add_argument("--allow-unbalanced", action="store_true", help="Allow classes to be unbalanced for metric computation.")
    vm.add_argument("--max-sites-per-read", type=int, help="Maximum number of sites to extract from a single read.")
    vm.add_argument("--seed", type=int,
                    help="Seed value. Default: Random seed.  Applied (np.random.seed) before anything is drawn, so that the sites "
                         "drawn under --max-sites-per-read and the balancing repeat; the reference logs its seed without applying it")
    vm.add_argument("--extra-bases", help="Extra canonical or modified base single letter codes not in the ground truth bed files "
                                          "which should be added to the accepted alphabet, e.g. `--extra-bases mh` for a canonical "
                                          "ground truth (C) and 5mC and 5hmC calls")
    vm.add_argument("--log-filename", help="Log filename. (default: Don't output log file)")
    vm.add_argument("--explicit-mod-tag-used", action="store_true",
                    help="Specify that the user has checked that the modified base tag (MM) uses the explicit (`?`) specifier")
    vm.add_argument("--device", type=int, default=0)
    vm.set_defaults(func=_validate_modbams)

    dset = sub.add_parser("dataset").add_subparsers(dest="sub", required=True)
    d = dset.add_parser("prepare", help="POD5 + BAM -> labelled chunk dataset directory")
    d.add_argument("pod5", help=POD5_HELP)
    d.add_argument("bam")
    d.add_argument("--output-path", default="remora_training_dataset")
    d.add_argument("--overwrite", action="store_true")
    d.add_argument("--motif", nargs=2, action="append", metavar=("MOTIF", "FOCUS_POSITION"), required=True)
    d.add_argument("--focus-reference-positions")
    d.add_argument("--chunk-context", default=list(constants.DEFAULT_CHUNK_CONTEXT), type=int, nargs=2)
    d.add_argument("--min-samples-per-base", type=int, default=constants.DEFAULT_MIN_SAMPLES_PER_BASE)
    d.add_argument("--kmer-context-bases", nargs=2, default=list(constants.DEFAULT_KMER_CONTEXT_BASES), type=int)
    d.add_argument("--max-chunks-per-read", type=int, default=15)
    d.add_argument("--base-start-justify", action="store_true")
    d.add_argument("--offset", default=0, type=int)
    d.add_argument("--num-reads", type=int)
    d.add_argument("--basecall-anchor", action="store_true")
    d.add_argument("--reverse-signal", action="store_true")
    d.add_argument("--save-every", default=100_000, type=int)
    d.add_argument("--skip-shuffle", action="store_true")
    d.add_argument("--refine-kmer-level-table")
    d.add_argument("--refine-rough-rescale", action="store_true")
    d.add_argument("--refine-scale-iters", default=-1, type=int)
    d.add_argument("--refine-half-bandwidth", default=5, type=int)
    d.add_argument("--refine-algo", default="dwell_penalty", choices=("Viterbi", "dwell_penalty"))
    d.add_argument("--refine-short-dwell-parameters", default=[4, 3, 0.5], type=float, nargs=3)
    d.add_argument("--rough-rescale-method", default="least_squares", choices=("least_squares", "theil_sen"))
    d.add_argument("--mod-base", nargs=2, metavar=("SHORT_NAME", "LONG_NAME"))
    d.add_argument("--mod-base-control", action="store_true")
    d.add_argument("--reads-per-batch", type=int, default=512)
    d.add_argument("--device", type=int, default=0)
    d.add_argument("--gpus", type=int, default=1,
                   help="one process per GPU, each extracts the chunks of its own share of the BAM; the parts become one dataset")
    d.add_argument("--procs-per-gpu", type=int, default=1, help="processes per GPU, each with its own share of the BAM (and, for a directory "
                                                                 "of POD5 files, its own read-id index)")
    d.set_defaults(func=_dataset_prepare)
    di = dset.add_parser("inspect", help="Summary of a dataset directory or config")
    di.add_argument("remora_dataset_path")
    di.add_argument("--out-path", help="write the expanded config (with hashes) here")
    di.set_defaults(func=_dataset_inspect)
    dm = dset.add_parser("make_config", help="Config drawing from several datasets at fixed proportions (no data copied)")
    dm.add_argument("out_path")
    dm.add_argument("dataset_paths", nargs="+")
    dm.add_argument("--dataset-weights", type=float, nargs="+")
    dm.set_defaults(func=_dataset_make_config)

    dg = dset.add_parser("merge", help="Copy several datasets into one new core dataset (shuffled)")
    dg.add_argument("out_path")
    dg.add_argument("dataset_paths", nargs="+")
    dg.add_argument("--max-size", type=int)
    dg.add_argument("--overwrite", action="store_true")
    dg.set_defaults(func=_dataset_merge)
    dh = dset.add_parser("head", help="New core dataset from the first chunks of another")
    dh.add_argument("out_path")
    dh.add_argument("in_path")
    dh.add_argument("num_chunks", type=int)
    dh.add_argument("--overwrite", action="store_true")
    dh.set_defaults(func=_dataset_head)
    dc = dset.add_parser("copy", help="Copy a dataset (all its core datasets + a new config) to a new location")
    dc.add_argument("in_path")
    dc.add_argument("out_path")
    dc.add_argument("--overwrite", action="store_true")
    dc.set_defaults(func=_dataset_copy)

    ana = sub.add_parser("analyze").add_subparsers(dest="sub", required=True)
    k = ana.add_parser("estimate_kmer_levels", help="Estimate k-mer level table (per-base trimmed means and both medians on the GPU)")
    k.add_argument("--pod5-and-bam", required=True, nargs=2, metavar=("POD5", "BAM"), action="append",
                   help="POD5 signal path (a file, or a run's directory of *.pod5 files as for infer from_pod5_and_bam) and BAM path; the BAM holds mapped reads with move tables and MD tags (no index needed); "
                        "repeat for several samples, which are aggregated after the site level")
    k.add_argument("--refine-kmer-level-table")
    k.add_argument("--refine-rough-rescale", action="store_true")
    k.add_argument("--refine-scale-iters", default=0, type=int)
    k.add_argument("--refine-half-bandwidth", default=5, type=int)
    k.add_argument("--refine-algo", default="dwell_penalty", choices=("Viterbi", "dwell_penalty"))
    k.add_argument("--refine-short-dwell-parameters", default=[4, 3, 0.5], type=float, nargs=3, metavar=("TARGET", "LIMIT", "WEIGHT"))
    k.add_argument("--min-coverage", type=int, default=10, help="Minimum coverage to include a site.")
    k.add_argument("--kmer-context-bases", nargs=2, default=(2, 2), type=int, metavar=("BASES_BEFORE", "BASES_AFTER"))
    k.add_argument("--levels-filename", default="remora_kmer_levels.txt")
    k.add_argument("--log-filename")
    k.add_argument("--num-workers", type=int, default=1, help="accepted for the reference's command lines; ignored")
    k.add_argument("--chunk-width", type=int, default=1_000, help="accepted for the reference's command lines; ignored")
    k.add_argument("--max-chunk-coverage", type=int, default=100, help="accepted for the reference's command lines; ignored")
    k.add_argument("--reverse-signal", action="store_true",
                   help="the signal was recorded 3'->5' (direct RNA): build the reads as models with reverse_signal read them. "
                        "The reference's get_site_kmer_levels takes this argument, its command line does not expose it")
    k.add_argument("--reads-per-batch", type=int, default=256)
    k.add_argument("--levels-device-gib", type=float, default=64.0,
                   help="GiB of GPU memory the bases aggregated at a time may take (capped at half of what is free): an input that "
                        "needs more is aggregated one range of reference sites after the other, each with a pass of its own over "
                        "the input (same table, any input size)")
    k.add_argument("--device", type=int, default=0)
    k.set_defaults(func=_estimate_kmer_levels)

    pm = ana.add_parser("pileup_modbams", help="Per-site modified-base counts (bedMethyl) from the MM/ML calls of mapped BAM files: tags "
                                               "tokenised on native threads; calls aligned, classified, sorted and counted per site on the GPU")
    pm.add_argument("--bam", required=True, action="append",
                    help="mapped BAM file with modified base tags; no index, sort order or MD tag needed; repeat to pile several files "
                         "(mapped to one reference) into one table")
    pm.add_argument("--out-bed", required=True, help="bedMethyl output: the eleven ENCODE columns, no header")
    pm.add_argument("--canonical-base", required=True, choices=list("ACGTU"), help="the canonical base of the modified bases counted")
    pm.add_argument("--mod-bases", required=True, nargs="+", metavar="CODE", help="one to seven single-letter modified-base codes, e.g. m h")
    pm.add_argument("--filter-threshold", type=float, help="a call passes when its winning probability is at least this (0 to 1)")
    pm.add_argument("--pct-filt", type=float,
                    help="filter this percentage (or less given ties) of the calls, the least confident ones, found in a first pass "
                         "over the input (default 10 when --filter-threshold is not given)")
    pm.add_argument("--min-coverage", type=int, default=1, help="write a site when at least this many of its calls pass")
    pm.add_argument("--counts-filename", help="TSV of the per-site counts of every class and of the failing calls")
    pm.add_argument("--region", help="ctg or ctg:start-end (0-based, half-open): only calls on these reference positions")
    pm.add_argument("--ref", metavar="FASTA",
                    help="the reference the reads were mapped to, plain FASTA with lines of one width per contig (no .fai needed): with "
                         "--motif or --cpg only calls on a motif of the reference are counted; it is packed into half a byte per base "
                         "of GPU memory")
    pm.add_argument("--motif", nargs=2, action="append", metavar=("MOTIF", "FOCUS_POSITION"),
                    help="count only calls whose reference position shows this IUPAC motif, the called base at FOCUS_POSITION (0-based); "
                         "up to 4 motifs of up to 16 bases; needs --ref")
    pm.add_argument("--cpg", action="store_true", help="--motif CG 0 (needs --canonical-base C)")
    pm.add_argument("--combine-strands", action="store_true",
                    help="one row per motif site with the calls of both strands, at the '+' position of the motif, strand column '.'; "
                         "every motif must be its own reverse complement (CG, GC, GATC)")
    pm.add_argument("--partition-tag", metavar="TAG", type=_partition_tag,
                    help="one table per value of this aux tag of the records (HP: per haplotype of phased reads), in one run and with "
                         "the one threshold of the whole input: --out-bed and --counts-filename become templates, s.bed -> s.TAG_1.bed, "
                         "s.TAG_2.bed, ..., s.ungrouped.bed for the records without the tag; integer (c C s S i I) or character (A) "
                         "values, up to 255 distinct ones")
    pm.add_argument("--duplex", action="store_true",
                    help="count the '-'-strand MM entries too (the G-m? part `infer duplex_from_pod5_and_bam` writes from the complement "
                         "read): such a call lies on the reference strand opposite to its record's")
    pm.add_argument("--hemi", action="store_true",
                    help="one row per motif site with the counts of the strand pairs of duplex records - both strands modified, either "
                         "one, neither: the '+' and the '-' call of one record at one site are a pair, named <+ class>,<- class>,<canonical "
                         "base> in the bedMethyl (m,m,C  m,-,C  -,m,C  -,-,C), columns N_<a>_<b> in --counts-filename; implies --duplex "
                         "and the fold of --combine-strands; needs --ref, one motif that is its own reverse complement (--cpg) and at "
                         "most two --mod-bases")
    pm.add_argument("--coverage-columns", action="store_true",
                    help="the eighteen-column bedMethyl: N_mod N_canonical N_other_mod N_delete N_fail N_diff N_nocall behind the eleven "
                         "columns, and N_delete N_diff N_nocall behind N_fail in --counts-filename.  Costs one more pass over the BAMs "
                         "once the table is finished - every record is joined on the GPU against the sites it spans: a deletion "
                         "there, another base than the canonical one, or the canonical base without a call - and 12 bytes of GPU "
                         "memory per site; not with --duplex or --hemi")
    pm.add_argument("--pileup-device-gib", type=float, default=8.0,
                    help="GiB of GPU memory for the call buffer and its sort (capped at half of what is free); the per-site table "
                         "comes on top, 8 + 4 (classes + 1) bytes per distinct site")
    pm.add_argument("--reads-per-batch", type=int, default=512)
    pm.add_argument("--device", type=int, default=0)
    pm.add_argument("--log-filename")
    pm.set_defaults(func=_pileup_modbams)
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    nranks = getattr(args, "gpus", 1) * max(getattr(args, "procs_per_gpu", 1), 1)
    if nranks > 1 and "WORLD_SIZE" not in os.environ:
        from .dist import launch_ranks

        by_scan = os.environ.get("REMORA_AMD_BAM_SHARD", "bytes") == "scan"
        scan_bam = args.in_bam if args.func is _infer and by_scan else None
        return launch_ranks(sys.argv[1:] if argv is None else list(argv), nranks, scan_bam=scan_bam)
    try:
        return args.func(args)
    except RemoraError as e:
        print(f"remora_amd: {e}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
