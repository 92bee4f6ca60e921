/*
 * Progress and cancellation of ONE file-level native call (GsGpuNative.hostMatchRun, hostFilterFiles, ...): what
 * AbstractLoggingFastqStreamer.doUpdateProgress / done / allDone (fastq/AbstractLoggingFastqStreamer.java:161-209, 247-252) do
 * around the reference's parser loop, for a pipeline that runs below the JVM.  SOURCE ONLY -- not compiled in the build container
 * (no JDK); tools/check_java_glue.py checks every reference member used here against the reference's sources.  See INTEGRATION.md.
 *
 * The constructor creates a control (gs_host_control_create) and attaches it to the calling thread -- the thread that makes the
 * native call next.  The native side never calls back into the JVM: a daemon thread takes a snapshot every updateMs milliseconds
 * and forwards it to bundle.setFastqProgress (the resource at the record's file index) and bundle.setTotalProgress with the
 * reference's argument meanings, and cancels the control when the calling thread has been interrupted
 * (FastqReaderInterruptedException is what the reference's readers throw then: translate()).  close() stops the thread, forwards the
 * last record, sends the final setTotalProgress as allDone() does, detaches and destroys the control.
 *
 *     GpuProgress progress = bundle.isRequiresProgress() ? new GpuProgress(bundle, resources, updateMs) : null;
 *     try {
 *         GsGpuNative.hostMatchRun(...);
 *     } catch (RuntimeException e) {
 *         throw GpuProgress.translate(e);
 *     } finally {
 *         if (progress != null) progress.close();
 *     }
 */
package org.metagene.genestrip.gpu;

import org.metagene.genestrip.ExecutionContext;
import org.metagene.genestrip.fastq.FastqReaderInterruptedException;
import org.metagene.genestrip.io.StreamingResource;

public final class GpuProgress {
	private final long control;
	private final ExecutionContext bundle;
	private final StreamingResource[] resources;
	private final int updateMs;
	private final Thread caller;
	private final Thread poller;
	private final long[] snapshot = new long[GsGpuNative.SNAPSHOT_LEN];
	private volatile boolean stop;

	public GpuProgress(ExecutionContext bundle, StreamingResource[] resources, int updateMs) {
		this.bundle = bundle;
		this.resources = resources;
		this.updateMs = Math.max(1, updateMs);
		caller = Thread.currentThread();
		control = GsGpuNative.hostControlCreate();
		GsGpuNative.hostControlAttach(control);
		poller = new Thread(this::poll, "gsgpu-progress");
		poller.setDaemon(true);
		poller.start();
	}

	private void poll() {
		while (!stop) {
			forward();
			if (caller.isInterrupted()) { // (the flag stays set: the caller sees it when the native call has returned)
				GsGpuNative.hostControlCancel(control);
			}
			try {
				Thread.sleep(updateMs);
			} catch (InterruptedException e) {
				return;
			}
		}
	}

	/** the latest record as doUpdateProgress reports it; false: no record yet */
	private synchronized boolean forward() {
		GsGpuNative.hostControlSnapshot(control, snapshot);
		if (snapshot[GsGpuNative.S_N_FILES] == 0) {
			return false;
		}
		int file = (int) snapshot[GsGpuNative.S_FILE];
		long bytes = snapshot[GsGpuNative.S_FILE_BYTES_DONE], size = snapshot[GsGpuNative.S_FILE_BYTES_TOTAL];
		long diff = snapshot[GsGpuNative.S_FILE_MS];
		double ratio = size <= 0 ? -1 : bytes / (double) size;
		double totalTime = ratio <= 0 ? -1 : diff / ratio;
		if (file >= 0 && file < resources.length) {
			bundle.setFastqProgress(resources[file], bytes, size, diff, (long) totalTime, ratio, snapshot[GsGpuNative.S_FILE_READS]);
		}
		bytes = snapshot[GsGpuNative.S_TOTAL_BYTES_DONE];
		size = snapshot[GsGpuNative.S_TOTAL_BYTES_TOTAL];
		diff = snapshot[GsGpuNative.S_TOTAL_MS];
		ratio = size <= 0 ? -1 : bytes / (double) size;
		totalTime = ratio <= 0 ? -1 : diff / ratio;
		bundle.setTotalProgress(bytes, size, diff, (long) totalTime, ratio, snapshot[GsGpuNative.S_TOTAL_READS],
				(int) snapshot[GsGpuNative.S_FILES_DONE], (int) snapshot[GsGpuNative.S_N_FILES]);
		return true;
	}

	public void close() {
		stop = true;
		poller.interrupt();
		boolean interrupted = false;
		for (;;) {
			try {
				poller.join();
				break;
			} catch (InterruptedException e) {
				interrupted = true;
			}
		}
		if (forward()) { // allDone(): covered == estimated, ratio 1
			long bytes = snapshot[GsGpuNative.S_TOTAL_BYTES_DONE], ms = snapshot[GsGpuNative.S_TOTAL_MS];
			bundle.setTotalProgress(bytes, bytes, ms, ms, 1, snapshot[GsGpuNative.S_TOTAL_READS], (int) snapshot[GsGpuNative.S_FILES_DONE],
					(int) snapshot[GsGpuNative.S_N_FILES]);
		}
		GsGpuNative.hostControlAttach(0);
		GsGpuNative.hostControlDestroy(control);
		if (interrupted) {
			Thread.currentThread().interrupt();
		}
	}

	/** the exception of a stopped call as the reference's readers throw it; any other as it is */
	public static RuntimeException translate(RuntimeException e) {
		return GsGpuNative.isCancelled(e) ? new FastqReaderInterruptedException() : e;
	}
}
