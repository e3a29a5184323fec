package lgbt.princess.reservoir.gpu

import scala.collection.immutable.ArraySeq
import scala.collection.mutable
import scala.reflect.ClassTag

import lgbt.princess.reservoir.Sampler

/** The downcalls an [[ObjectDistinct]] makes: the hash-only candidate pass (include/reservoir_hip.h
  * rsv_distinct_candidates / rsv_candidates_read / rsv_candidates_commit / rsv_candidates_abort) and
  * the handle's release.  The JNI binding implements it over `Jni` (JniSampler.scala), the FFM
  * binding over its downcall handles (FfmSampler.scala). */
private[reservoir] trait CandidateOps {

  /** the next n elements by hash alone (hashes(0 until n) = hash(map(x))); returns the candidate count */
  def candidates(hashes: Array[Long], n: Int): Int

  /** the pending batch's c candidates: offsets ascending in [0, n), scrambled hashes beside them */
  def read(offsets: Array[Long], scrambled: Array[Long], c: Int): Unit

  /** accept the pending batch; setSize / maxHash = this replica after replaying the candidates */
  def commit(setSize: Int, maxHash: Long): Unit

  /** drop the pending batch */
  def abort(): Unit

  /** destroy the handle (a single-use result(), or the cleaner) */
  def release(): Unit
}

/** A GPU-backed `Sampler.distinct[A, B]` for ANY `B` (a String, a case class, a tuple:
  * Sampler.scala:171-180 takes every `B` with a ClassTag), where `B` has no fixed-width key the engine
  * could store.
  *
  * RandomValues.sample needs the element itself only for `elements.contains` (Sampler.scala:398, :403);
  * the admission test `elemHash < maxHash` needs only the hash.  So `hash(map(x))` is evaluated here
  * per element into a batch buffer, the engine reads the hashes alone (8 B per element) and returns
  * the few batch positions the reference could still admit -- a superset of its admissions, in
  * arrival order, with the scrambled hashes of Sampler.scala:396 -- and this class replays
  * RandomValues.sample over those elements only.  It holds `mutable.PriorityQueue[(B, Long)]` and
  * `mutable.Set[B]` exactly as the reference does (Sampler.scala:389-392), so the tie order of an
  * oversubscribed boundary hash bucket is the reference's own.  r0 / r1 live in the engine, seeded per
  * sampler like `new Random()` (Sampler.scala:385-388).
  *
  * Every downcall after `candidates` runs under try / abort: a failure drops the batch on both sides
  * (the engine's count, shadow and bound; this buffer), the sampler stays usable and the error
  * propagates.
  *
  * tests/cpp/test_object_distinct.cpp (ObjectDistinctMirror) replays this class's downcalls on the GPU. */
private[reservoir] final class ObjectDistinct[A, B: ClassTag](maxSampleSize: Int, reusable: Boolean, ops: CandidateOps)(
    map: A => B,
    hash: B => Long,
) extends Sampler[A, B] {
  private[this] final val Batch = 65536
  private[this] val samples: mutable.PriorityQueue[(B, Long)] =
    mutable.PriorityQueue.empty[(B, Long)](Ordering.by(_._2))
  private[this] val elements: mutable.Set[B] = mutable.Set.empty
  private[this] var maxHash                  = Long.MinValue
  private[this] val pending                  = new Array[AnyRef](Batch) // map(x) of the buffered elements, boxed
  private[this] val hashes                   = new Array[Long](Batch)   // hash(map(x))
  private[this] var n                        = 0
  private[this] var offsets                  = new Array[Long](1024)
  private[this] var scrambled                = new Array[Long](1024)
  private[this] var open                     = true

  /** RandomValues.sample (Sampler.scala:397-408) for an element already mapped and scrambled */
  private[this] def replay(elem: B, elemHash: Long): Unit =
    if (samples.size < maxSampleSize) {
      if (!elements.contains(elem)) {
        samples += ((elem, elemHash))
        elements += elem
        maxHash = maxHash max elemHash
      }
    } else if (elemHash < maxHash && !elements.contains(elem)) {
      elements -= samples.dequeue()._1
      samples += ((elem, elemHash))
      elements += elem
      maxHash = samples.head._2
    }

  /** the buffered elements as one engine batch; the buffer is empty afterwards, whatever happens */
  private[this] def flush(): Unit =
    if (n > 0) {
      val len = n
      try {
        val c = ops.candidates(hashes, len)
        try {
          if (offsets.length < c) {
            offsets = new Array[Long](c)
            scrambled = new Array[Long](c)
          }
          ops.read(offsets, scrambled, c)
        } catch {
          case t: Throwable => // nothing replayed yet: drop the batch on the engine's side too
            try ops.abort()
            catch { case e: Throwable => t.addSuppressed(e) }
            throw t
        }
        var i = 0
        while (i < c) {
          replay(pending(offsets(i).toInt).asInstanceOf[B], scrambled(i))
          i += 1
        }
        // A failing commit must not leave the batch pending.  Dropping it on the engine's side is
        // sound although the replica has replayed it: the engine's bound only loosens (its earlier
        // shadow and the earlier maxHash still bound the replica's maxHash from above).
        try ops.commit(samples.size, maxHash)
        catch {
          case t: Throwable =>
            try ops.abort()
            catch { case e: Throwable => t.addSuppressed(e) }
            throw t
        }
      } finally {
        java.util.Arrays.fill(pending, 0, len, null) // let the elements go
        n = 0
      }
    }

  def sample(element: A): Unit = {
    if (!open) throw new IllegalStateException(Abi.ClosedMessage)
    val elem = map(element)
    hashes(n) = hash(elem)
    pending(n) = elem.asInstanceOf[AnyRef]
    n += 1
    if (n == Batch) flush()
  }

  def result(): IndexedSeq[B] = {
    if (!open) throw new IllegalStateException(Abi.ClosedMessage)
    flush()
    val res = elements to ArraySeq // Sampler.scala:411
    if (!reusable) {
      open = false
      ops.release()
    }
    res
  }

  def isOpen: Boolean = open
}
