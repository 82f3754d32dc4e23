"""What trainV1_warmup and trainV2_simt share around the trainers' step(), for all three --model values: `setup_devices` (this rank's GPU
and the RCCL group) and `train`, the outer loop of the reference (trainV1_warmup.py:206-256, trainV2_simt.py:307-464) -- resume, step, loss
line, final snapshot, evaluation or rolling snapshot, train state, shutdown.  The tools hand `train` what differs between them: the
snapshots' stem, the step arguments, the loss line and the evaluation (`scorer`)."""
import os
import os.path as osp
import time

import torch

from simt_amd.train_state import save_atomic


def setup_devices(args, needs_gpu):
    """-> (rank, world, device, process group or None): this rank's GPU and, under torchrun (WORLD_SIZE > 1), the RCCL group.
    needs_gpu: the tool's exit message on a machine without one."""
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", str(args.gpu)))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if not torch.cuda.is_available():
        raise SystemExit(needs_gpu)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    pg = None
    if world > 1:
        import torch.distributed as dist
        from simt_amd.engine import reserve_streams
        reserve_streams(dev)                                    # the plan's streams take their hardware queues before RCCL makes its own
        os.environ.setdefault("NCCL_MAX_NCHANNELS", "16")      # the conv tile lists leave 20 CUs to the collective's kernels (engine.TrunkPlan.cu_budget)
        dist.init_process_group("nccl", device_id=dev)
        pg = dist.group.WORLD
    return rank, world, dev, pg


def shutdown(world):
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def scorer(args, tr, open_classes, dev, rank, world, pg, **model):
    """-> make_score of `train` for both tools: at its first call ONE Evaluator over the trainer's parameters (--eval-dtype), then
    evaluate_simt through it -- with open_classes 0 that is evaluate_warmup.  model: the Evaluator's model= / layers= of a one-output model."""
    def make_score():
        from simt_amd.tools.evaluate_cityscapes import Evaluator, evaluate_simt
        kw = dict(num_classes=args.num_classes, open_classes=open_classes, device=dev,
                  dtype=torch.bfloat16 if args.eval_dtype == "bf16" else torch.float32, **model)
        evaluator = Evaluator(tr.params, **kw)
        return lambda params: evaluate_simt(params, args.data_dir_val, args.data_list_val, args.gt_dir_val, args.devkit_dir,
                                            evaluator=evaluator, rank=rank, world=world, process_group=pg, **kw)
    return make_score


def train(args, tr, stem, cd, rank, world, open_data, loss_line, make_score):
    """The loop of both tools over the trainer `tr`, from the snapshot rotation `<stem><i>...pth` to the shutdown.
    open_data(start_batch) -> next_step, called once the start iteration is known (0, or --train-state's): it creates the loaders at this
    rank's batch start_batch; next_step() -> (args, kwargs) of tr.step(*args, i_iter, **kwargs), one iteration's iter_size micro-batches.
    loss_line(i_iter, losses, rate) -> the line rank 0 prints every --print-every iterations, rate in images per second.
    make_score() -> score(params) -> mIoU: called at the first evaluation, and only with --data-dir-val (it builds the one Evaluator)."""
    from simt_amd.tools.trainV2_simt import EmaSnapshots, SnapshotKeeper, TrainStateFile      # (not at the top: that module imports this one)
    score, keeper = None, SnapshotKeeper(args.snapshot_dir, stem)
    resume = TrainStateFile(args, rank, world, cd)
    ema_snap = EmaSnapshots(tr, keeper, resume, rank)
    start = resume.resume(tr, keeper)
    if resume.complete(start, args.num_steps_stop, tr, args.snapshot_dir):
        return shutdown(world)
    next_step = open_data(start * args.iter_size)
    t0 = time.time()
    for i_iter in range(start, args.num_steps):
        a, kw = next_step()
        tr.step(*a, i_iter, **kw)
        if i_iter % args.print_every == 0:              # trainV1_warmup.py:231-234, trainV2_simt.py:438-441 (every 100 iterations there)
            l = tr.losses()                        # every rank (DP: a bad-label error is raised on all of them together)
            if rank == 0:
                print(loss_line(i_iter, l, args.batch_size * world * (i_iter + 1 - start) / max(time.time() - t0, 1e-9)))
        if i_iter >= args.num_steps_stop - 1:                         # trainV1_warmup.py:236-239, trainV2_simt.py:447-450
            if rank == 0:
                print("save model ...")
                save_atomic(tr.state_dict(), osp.join(args.snapshot_dir, "GTA5_" + str(args.num_steps_stop) + ".pth"))
            ema_snap.final(args.snapshot_dir, args.num_steps_stop)
            resume.write(tr, keeper)
            break
        if i_iter % args.save_pred_every == 0 and i_iter != 0 and args.data_dir_val:
            # trainV1_warmup.py:241-256, trainV2_simt.py:452-464: evaluate on the validation set, keep only the best-mIoU snapshot
            # `<stem><i>_mIoU<m>.pth`
            if score is None:
                score = make_score()
            if rank == 0:
                print(time.strftime("%Y-%m-%d %H:%M:%S"), "  Begin evaluation on iter {0:8d}/{1:8d}  ".format(i_iter, args.num_steps))
            mIoU = score(tr.params)
            if rank == 0:
                print("Finish Evaluation: " + time.asctime(time.localtime(time.time())))
                keeper.best(tr.state_dict(), i_iter, mIoU)
            ema_snap.evaluated(score, i_iter)          # --ema: the averaged model through the same Evaluator, a rotation of its own
        elif i_iter % args.save_pred_every == 0 and i_iter != 0 and rank == 0:
            # no validation set given (the reference hard-codes one, evaluate_cityscapes.py:26-28; :452-464): without an evaluation there is
            # no best-mIoU snapshot, so keep a rolling periodic one -- a crash must not lose the run
            keeper.rolling(tr.state_dict(), i_iter)
            ema_snap.rolling(i_iter)
        resume.after_iteration(i_iter, tr, keeper)
    shutdown(world)
