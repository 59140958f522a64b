/*
 * fury_row.h — C ABI of the MI355X-native Fury row-format codec.
 *
 * This is the drop-in boundary for the hot path named by BASELINE.json `north_star`:
 * java/fury-format's row encode/decode and row -> Arrow-column conversion.  Java objects
 * cannot cross onto the device, so the boundary is batches of Arrow-style columns <-> batches
 * of Fury rows; every row's bytes are identical to what the reference writes for the same
 * field values (see DESIGN.md "Parity").
 *
 * Reference interfaces each entry point replaces (paths relative to the reference root,
 * FMT = java/fury-format/src/main/java/org/apache/fury/format):
 *
 *   fury_schema_create      TypeInference.inferSchema + BinaryRowWriter ctor layout
 *                           (FMT/type/TypeInference.java:64-76,136-238,
 *                            FMT/row/binary/writer/BinaryRowWriter.java:46-52)
 *   fury_schema_hash        DataTypes.computeSchemaHash (FMT/type/DataTypes.java:499-544)
 *   fury_type_width         DataTypes.getTypeWidth (FMT/type/DataTypes.java:68-133,225-227)
 *   fury_row_measure        the writerIndex growth of generated toRow
 *                           (FMT/encoder/RowEncoderBuilder.java:154-179) — row sizes + scan
 *   fury_row_encode         RowEncoder.toRow over a batch: generated toRow + BinaryRowWriter /
 *                           BinaryWriter / BinaryArrayWriter (FMT/encoder/Encoders.java:88-93,
 *                           FMT/encoder/BaseBinaryEncoderBuilder.java:138-453,
 *                           FMT/row/binary/writer/BinaryWriter.java:106-194,
 *                           FMT/row/binary/writer/BinaryRowWriter.java:76-124,
 *                           FMT/row/binary/writer/BinaryArrayWriter.java:77-118)
 *   fury_row_encode_measured both in one call (toRow into a growable buffer, Encoders.java:88-93)
 *   fury_row_decode_measure the Arrow offsets fromRow/ArrowWriter would produce
 *   fury_row_decode         RowEncoder.fromRow over a batch: BinaryRow getters
 *                           (FMT/encoder/RowEncoderBuilder.java:185-217,
 *                            FMT/row/binary/UnsafeTrait.java:68-197,
 *                            FMT/row/binary/BinaryArray.java:69-78,157-197)
 *   fury_row_project        BinaryRow.isNullAt / getInt64 / getString / getDecimal / getArray
 *   fury_row_project_measure  (ordinal) over a batch, for the selected ordinals only
 *                           (FMT/row/binary/BinaryRow.java getters,
 *                            FMT/row/binary/UnsafeTrait.java:68-197,
 *                            FMT/row/binary/BinaryArray.java:69-78)
 *   fury_row_update         BinaryRow.setBoolean / setByte / setInt16 / setInt32 / setInt64 /
 *                           setFloat32 / setFloat64 / setDate / setTimestamp / setNullAt /
 *                           setNotNullAt (ordinal) over a batch, for the selected ordinals only
 *                           (FMT/row/binary/UnsafeTrait.java:203-266,
 *                            FMT/row/binary/BinaryRow.java:130-150)
 *   fury_row_take /         BinaryRow.copy() over a batch, for the selected rows only: a row's bytes,
 *   fury_row_filter         unchanged, at a new position (FMT/row/binary/BinaryRow.java:173-179)
 *   fury_row_extract        BinaryRow.getStruct / getArray / getMap (ordinal) over a batch, along a path
 *                           of struct ordinals: the nested row / BinaryArray / BinaryMap of every row
 *                           as a batch of the child schema (fury_schema_child)
 *                           (FMT/row/binary/UnsafeTrait.java:160-197,
 *                            FMT/row/binary/BinaryMap.java:62-77)
 *   fury_row_explode        BinaryArray.getStruct / getArray / getMap (ordinal) and BinaryMap.keyArray /
 *                           valueArray over a batch: the elements of a list or map field of every row
 *                           as a batch of the element schema (fury_schema_element)
 *                           (FMT/row/binary/BinaryArray.java:137-150,
 *                            FMT/row/binary/BinaryMap.java:101-108)
 *   fury_row_select         BinaryRow getters feeding BinaryRowWriter.write(ordinal, <primitive>) /
 *                           BinaryWriter.writeUnaligned / write(ordinal, BinaryRow | BinaryArray |
 *                           BinaryMap) -> writeAlignedBytes / copyTo over a batch: a subset of every
 *                           row's fields as rows of the selected schema (fury_schema_select)
 *                           (FMT/row/binary/writer/BinaryWriter.java:161-212,243-245,
 *                            FMT/row/binary/writer/BinaryRowWriter.java:86-129)
 *   fury_row_zip            the same writer calls fed from the getters of several BinaryRows: the fields
 *                           of up to four batches joined row by row, as rows of the zipped schema
 *                           (fury_schema_zip)
 *   fury_row_implode        BinaryArrayWriter.reset(n) + write(ordinal, BinaryRow | BinaryArray |
 *                           BinaryMap) / setNullAt over a batch: element rows back into the LIST of
 *                           every row, the inverse of fury_row_explode
 *                           (FMT/row/binary/writer/BinaryArrayWriter.java:91-129,
 *                            FMT/row/binary/writer/BinaryWriter.java:106-114,243-245)
 *   fury_row_wrap           BinaryRowWriter.write(0, BinaryRow | BinaryArray | BinaryMap) over a batch:
 *                           nested values back into one-field rows, the inverse of fury_row_extract
 *   fury_rows_to_arrow    ArrowWriter.write(row)* + finishAsRecordBatch
 *                           (FMT/vectorized/ArrowWriter.java:74-99,205-225,519-540)
 *   fury_arrow_append       ArrowWriter.write(row) appending at rowCount until finish() / reset()
 *                           (FMT/vectorized/ArrowWriter.java:74-99)
 *   fury_frame_rows /       RowEncoder.encode(MemoryBuffer, T) / decode(MemoryBuffer) stream
 *   fury_unframe_rows       framing [int32 len][int64 schemaHash][row]
 *                           (FMT/encoder/Encoders.java:165-182,201-213)
 *
 * Conventions
 *   - Every function returns an int status (FURY_OK == 0).  On failure a message is kept per
 *     thread and can be read with fury_last_error().  Status codes map 1:1 onto the
 *     reference's exception types (see fury_status).
 *   - Pointers passed to the fury_row_* / fury_rows_* / fury_*frame* functions are DEVICE
 *     pointers on the calling thread's current HIP device; `stream` is a hipStream_t (NULL =
 *     the legacy default stream).  Calls are asynchronous on `stream` unless documented.
 *   - Arrow layout: validity bitmaps are LSB-first with bit = 1 meaning VALID (Arrow); the row
 *     bitmap inside a Fury row is LSB-first with bit = 1 meaning NULL (BitUtils.set,
 *     fury-core memory/BitUtils.java:36-43,175-177).  All integers little-endian, floats as raw
 *     bits (MemoryBuffer.putFloat64 = doubleToRawLongBits).
 *   - Canonical bytes are the fresh-buffer bytes of RowEncoder.toRow(obj) (Encoders.java:88-93):
 *     a null field's slot is 0.  See DESIGN.md "Null slots" for RowEncoder.encode(obj)'s reused
 *     buffer.
 */
#ifndef FURY_ROW_H_
#define FURY_ROW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FURY_ROW_ABI_VERSION 1

/* Status codes; the reference exception each one stands for is named. */
typedef enum fury_status {
  FURY_OK = 0,
  FURY_ERR_INVALID_ARGUMENT = 1,       /* IllegalArgumentException / checkArgument          */
  FURY_ERR_UNSUPPORTED = 2,            /* UnsupportedOperationException
                                          (TypeInference.java:233-237, BinaryArrayWriter.java:99-101) */
  FURY_ERR_CLASS_NOT_COMPATIBLE = 3,   /* ClassNotCompatibleException (Encoders.java:170-178) */
  FURY_ERR_OUT_OF_BOUNDS = 4,          /* IndexOutOfBoundsException (MemoryBuffer bounds)    */
  FURY_ERR_ENCODER = 5,                /* EncoderException (Encoders.java:215-218)          */
  FURY_ERR_DEVICE = 6,                 /* HIP runtime failure (no reference equivalent)     */
  FURY_ERR_CAPACITY = 7                /* output buffer too small for measured bytes        */
} fury_status;

/* Type ids = org.apache.fury.format.type.ArrowType ids (FMT/type/ArrowType.java:25-148);
 * they are also the ids hashed by DataTypes.computeSchemaHash. */
typedef enum fury_type_id {
  FURY_TYPE_BOOL = 1,
  FURY_TYPE_INT8 = 3,
  FURY_TYPE_INT16 = 5,
  FURY_TYPE_INT32 = 7,
  FURY_TYPE_INT64 = 9,
  FURY_TYPE_FLOAT32 = 11,
  FURY_TYPE_FLOAT64 = 12,
  FURY_TYPE_STRING = 13,   /* Arrow utf8  */
  FURY_TYPE_BINARY = 14,
  FURY_TYPE_DATE32 = 16,
  FURY_TYPE_TIMESTAMP = 18, /* microseconds */
  FURY_TYPE_DECIMAL = 23,  /* decimal128, 16 bytes */
  FURY_TYPE_LIST = 25,
  FURY_TYPE_STRUCT = 26,
  FURY_TYPE_MAP = 30
} fury_type_id;

/* A schema field (a node of org.apache.arrow.vector.types.pojo.Field as built by
 * TypeInference.inferField).  Fields are given in slot order, i.e. already sorted the way
 * Descriptor orders bean fields (lexicographic Java field name, Descriptor.java:324-332);
 * fury_sort_bean_fields() performs that ordering. */
typedef struct fury_field {
  const char* name;
  int32_t type_id;                  /* fury_type_id                                    */
  int32_t nullable;                 /* FieldType.nullable                              */
  int32_t num_children;             /* LIST: 1 (element), STRUCT: n, MAP: 2 (key, value) */
  const struct fury_field* children;
} fury_field;

typedef struct fury_schema fury_schema; /* opaque, immutable after creation, thread-safe */

/* Arrow-style column (one per top-level field, in schema order).  Array offset is 0.
 *   fixed width : values = n * width bytes (BOOL: bit-packed, Arrow), validity optional
 *   STRING/BINARY: offsets = n+1 int32, values = payload bytes
 *   DECIMAL     : values = n * 16 bytes (decimal128 little-endian)
 *   LIST        : offsets = n+1 int32 element offsets, child = element column (flattened)
 *   STRUCT      : child = array of the struct's field columns (entry-aligned with the parent)
 *   MAP         : offsets = n+1 int32 entry offsets, child = [keys column, values column]
 * validity: encode input NULL = all valid; decode output NULL = do not write validity.
 * capacity: decode output only — bytes available in `values` (STRING/BINARY payload; for a LIST,
 *   the child column's capacity bounds its element values).  Decode never writes past it.
 * Decode output bitmaps (validity, BOOL values) are written as 32-bit words: 4-byte aligned,
 *   padded to a multiple of 4 bytes. */
typedef struct fury_column {
  void* values;
  uint8_t* validity;
  int32_t* offsets;
  int64_t capacity;
  struct fury_column* child;
} fury_column;

/* Describes the computed layout of a schema (BinaryRowWriter ctor, BinaryRowWriter.java:46-52). */
typedef struct fury_schema_info {
  int32_t num_fields;
  int32_t bitmap_bytes;   /* BitUtils.calculateBitmapWidthInBytes(numFields) */
  int32_t fixed_size;     /* bitmap_bytes + 8 * num_fields                   */
  int32_t is_fixed;       /* 1 when every field is fixed width: rows are fixed_size bytes */
  int64_t schema_hash;    /* DataTypes.computeSchemaHash                     */
} fury_schema_info;

/* ---- version / errors ---------------------------------------------------------------- */
int32_t fury_abi_version(void);
/* Copies the calling thread's last error message (NUL-terminated, truncated to len). */
size_t fury_last_error(char* buf, size_t len);

/* ---- schema (host) --------------------------------------------------------------------- */
/* DataTypes.getTypeWidth: byte width of a fixed-width type, -1 for variable-length types. */
int32_t fury_type_width(int32_t type_id);
/* Sort `n` field indices by Java field name the way Descriptor does (String.compareTo on
 * UTF-16 code units); writes the permutation to order[0..n). */
int fury_sort_bean_fields(const char* const* java_names, int32_t n, int32_t* order);
/* StringUtils.lowerCamelToLowerUnderscore (fury-core util/StringUtils.java:252-271).
 * Returns the length written (excluding NUL); out must hold 2*strlen(in)+1 bytes. */
int32_t fury_lower_camel_to_lower_underscore(const char* in, char* out, size_t out_len);
/* Any number of fields; nested STRUCT / LIST / MAP up to 64 levels and 4096 nodes (a deeper or
 * larger schema is created, and its encode / decode calls return FURY_ERR_UNSUPPORTED).  Every
 * row of a schema within those limits encodes and decodes on the device, whatever its size. */
int fury_schema_create(const fury_field* fields, int32_t num_fields, fury_schema** out);
void fury_schema_destroy(fury_schema* schema);
int fury_schema_get_info(const fury_schema* schema, fury_schema_info* info);

/* ---- device batch codec ---------------------------------------------------------------- */
/* Row sizes and their exclusive scan: row_offsets[0..nrows] (int64, device); row i occupies
 * [row_offsets[i], row_offsets[i+1]) and row_offsets[nrows] is the batch's byte total.
 * For is_fixed schemas this is optional (rows sit at i * fixed_size).
 *
 * Everywhere a function below takes `rows` with `row_offsets`, row_offsets[0] need not be 0: a batch
 * may sit anywhere in its buffer (an interior slice of a larger batch with its offsets as they are, a
 * batch encoded at row_offsets = measured + B), at byte positions past 2^31 and 2^32 alike, and every
 * bounds rule reads "inside [0, row_offsets[nrows])" -- the lower bound is the buffer's byte 0, not
 * row_offsets[0].  The one exception is fury_frame_rows, which places frame i at
 * row_offsets[i] + 12 * i and so is defined for batches whose offsets start at 0. */
int fury_row_measure(const fury_schema* schema, const fury_column* columns, int64_t nrows,
                     int64_t* row_offsets, void* stream);
/* Encode nrows rows into `rows` (device, 8-byte aligned, row_offsets[nrows] bytes, or
 * nrows * fixed_size when row_offsets is NULL and the schema is fixed). */
int fury_row_encode(const fury_schema* schema, const fury_column* columns, int64_t nrows,
                    const int64_t* row_offsets, void* rows, void* stream);
/* Measure + encode in one call with no host synchronisation — the batch form of toRow writing
 * into a growable buffer: writes row_offsets[0..nrows] exactly as fury_row_measure and the rows
 * into `rows`
 * (capacity bytes).  Bytes at or past `capacity` are never written: when row_offsets[nrows] >
 * capacity, grow the buffer and call again.  Fixed schemas know their size up front and return
 * FURY_ERR_CAPACITY instead (row_offsets may be NULL for them). */
int fury_row_encode_measured(const fury_schema* schema, const fury_column* columns, int64_t nrows,
                             int64_t* row_offsets, void* rows, int64_t capacity, void* stream);
/* Decode pass 1 for variable-length outputs: writes columns[i].offsets (STRING/BINARY/LIST)
 * and, for LIST, nothing else.  The caller reads offsets[nrows] to size values/child buffers. */
int fury_row_decode_measure(const fury_schema* schema, const void* rows,
                            const int64_t* row_offsets, int64_t nrows, fury_column* columns,
                            void* stream);
/* Decode rows into columns (RowEncoder.fromRow semantics: a null field leaves 0 bytes and,
 * when validity != NULL, a cleared validity bit).  One device pass: the STRING/BINARY/LIST
 * offsets are computed here (fury_row_decode_measure is only needed to size the buffers); when
 * offsets[nrows] exceeds a column's capacity the payload past the capacity is not written —
 * grow the buffer and decode again.  Malformed rows are reported asynchronously, on `stream`
 * (fury_device_status below).  Nested schemas, and flat ones with more than 256 fields of which
 * some are variable-length (the generic engine), decode through fury_decode_prepare /
 * fury_decode_execute instead: these calls (and fury_row_decode_measure) return
 * FURY_ERR_INVALID_ARGUMENT for them, naming the plan API. */
int fury_row_decode(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, fury_column* columns, void* stream);
/* ArrowWriter.write(row) for every row + finishAsRecordBatch: as fury_row_decode but every
 * column's validity is required (Arrow vectors always carry one) and null lists become
 * zero-length entries (ListVector fillHoles, ArrowWriter.java:539,223-225). */
int fury_rows_to_arrow(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, fury_column* columns, void* stream);

/* Projected decode -- BinaryRow's getters over a batch (isNullAt / getInt64 / getString /
 * getDecimal / getArray (ordinal): one bitmap bit and one 8-byte slot per field,
 * FMT/row/binary/BinaryRow.java getters, FMT/row/binary/UnsafeTrait.java:68-197, an array's header
 * BinaryArray.pointTo, FMT/row/binary/BinaryArray.java:69-78): decode only the top-level fields
 * fields[0..num_selected) (slot indices of `schema`, any order, no duplicates) into
 * columns[0..num_selected), in selection order.  Same column layout, alignment, capacity, error and
 * `arrow` semantics as fury_row_decode / fury_rows_to_arrow for the same field: a null field leaves
 * 0 bytes and a cleared validity bit, validity and BOOL bitmaps are written as whole 32-bit words,
 * payload at or past `capacity` is never written while offsets[nrows] holds the size needed, and a
 * selected value that lies outside the batch decodes as null and is reported on `stream`
 * (fury_device_status: FURY_ERR_OUT_OF_BOUNDS).  Only the bitmap words and slots of the selected
 * fields, and the bytes their values point at, are read: the schema may be flat, wide or nested,
 * and a corrupt slot of a field that is not selected is not an error.  A selected field must be a
 * fixed-width scalar, BOOL, STRING / BINARY, DECIMAL or a LIST of fixed-width (or BOOL) elements;
 * a STRUCT, MAP or LIST of variable-length elements returns FURY_ERR_UNSUPPORTED (decode those
 * with fury_decode_prepare / fury_decode_execute), as do a collection schema and more than 64
 * selected fields (run the full decode).  row_offsets may be NULL for is_fixed schemas (row i at
 * i * fixed_size).  Asynchronous on `stream`, no host synchronisation. */
int fury_row_project(const fury_schema* schema, const int32_t* fields, int32_t num_selected,
                     const void* rows, const int64_t* row_offsets, int64_t nrows,
                     fury_column* columns, int32_t arrow, void* stream);
/* Pass 1 for sizing: writes only columns[j].offsets of the selected STRING / BINARY / LIST fields
 * (as fury_row_decode_measure does for all fields). */
int fury_row_project_measure(const fury_schema* schema, const int32_t* fields, int32_t num_selected,
                             const void* rows, const int64_t* row_offsets, int64_t nrows,
                             fury_column* columns, void* stream);

/* In-place update -- BinaryRow's setters over a batch (setBoolean / setByte / setInt16 / setInt32 /
 * setInt64 / setFloat32 / setFloat64 / setDate / setTimestamp, FMT/row/binary/UnsafeTrait.java:203-266;
 * setNullAt / setNotNullAt, FMT/row/binary/BinaryRow.java:130-150): overwrite the top-level fields
 * fields[0..num_selected) (slot indices of `schema`, any order, no duplicates) of every row of
 * `rows` with the input columns columns[0..num_selected), in selection order.  Per row r and
 * selected field k of width w:
 *   value valid (validity NULL or bit r = 1)  setX(k, v): bit k of the row's null bitmap is cleared
 *       and bytes [0, w) of slot k become the little-endian value (BOOL: one byte, 0 or 1; floats as
 *       raw bits); bytes [w, 8) of the slot stay exactly as they were (0 in any row a writer made);
 *   value null (bit r = 0)                    setNullAt(k): bit k is set and the 8 slot bytes become 0;
 *   row_mask given and its bit r = 0          no byte of row r is written.
 * No other byte changes: other bits of the same bitmap word, other slots, the variable-length
 * section and padding are never rewritten.  So for rows made by fury_row_encode and no row_mask the
 * batch equals fury_row_encode of the original columns with the selected ones replaced.
 * columns[j] follows fury_row_encode's input contract for its field: values = nrows * width bytes,
 * aligned to the width (BOOL: bit-packed, Arrow), validity optional (NULL = all valid).  The BOOL
 * values, validity and row_mask bitmaps (LSB-first) are READ as 32-bit words: 4-byte aligned and
 * readable up to a multiple of 4 bytes.  `rows` is 8-byte aligned; row_offsets may be NULL for
 * is_fixed schemas (row i at i * fixed_size; a non-NULL row_offsets is ignored for them, as in
 * fury_row_project).  A selected field must be BOOL, INT8/16/32/64, FLOAT32/64, DATE32 or TIMESTAMP:
 * STRING / BINARY / DECIMAL / LIST / STRUCT / MAP return FURY_ERR_UNSUPPORTED (a variable-length
 * value cannot be updated in place: re-encode the batch), as do a collection schema and more than
 * 64 selected fields.  The rest of the schema may be anything (wide, nested, variable-length).
 * Bounds: row r is written only when [row_offsets[r], row_offsets[r] + fixed_size) lies inside
 * [0, row_offsets[nrows]) and row_offsets[r + 1] - row_offsets[r] >= fixed_size; otherwise no byte of
 * that row is written and FURY_ERR_OUT_OF_BOUNDS is reported on `stream` (fury_device_status).
 * Nothing outside the batch is ever written.  Rows that overlap through non-monotone offsets get
 * unspecified contents (never a write outside the batch).  Two updates of the same batch must be
 * ordered by the caller (same stream, or an event): fields can share a bitmap word, which each call
 * reads, merges and rewrites.  Asynchronous on `stream`, no host synchronisation; argument errors
 * are returned before any device work; nrows == 0 returns FURY_OK. */
int fury_row_update(const fury_schema* schema, const int32_t* fields, int32_t num_selected,
                    void* rows, const int64_t* row_offsets, int64_t nrows,
                    const fury_column* columns, const uint8_t* row_mask, void* stream);

/* Row selection -- BinaryRow.copy() over a batch (FMT/row/binary/BinaryRow.java:173-179:
 * buffer.copyTo(baseOffset, copyBuf, 0, sizeInBytes)).  Every (offset << 32) | size slot of a row is
 * relative to the row's own base, so a selected row is its bytes, unchanged, at a new position: only
 * row_offsets and bytes are used, and `schema` may be anything the library creates (flat, wide,
 * nested, a collection schema).
 *
 * fury_row_take: output row j = the bytes of source row indices[j], j in [0, num_selected).
 * `indices` is device int64 in any order, repeats allowed, num_selected may exceed nrows.
 * out_offsets[0..num_selected] (device) receives the exclusive scan of the selected rows' sizes;
 * out_offsets[num_selected] is the number of bytes the output needs.  Capacity as in
 * fury_row_encode_measured: output bytes at or past out_capacity are never written while out_offsets
 * is always complete, so the caller can grow the buffer and call again.  out_rows == NULL is the
 * measure form: only out_offsets is written (out_capacity is ignored).
 * is_fixed schemas: row_offsets may be NULL (a non-NULL one is ignored, as in fury_row_project),
 * output row j sits at j * fixed_size, out_offsets may be NULL (when given it is filled with
 * j * fixed_size), and out_rows != NULL with out_capacity < num_selected * fixed_size returns
 * FURY_ERR_CAPACITY before any device work.
 *
 * fury_row_filter: keeps the rows whose row_mask bit is 1, in row order.  row_mask is LSB-first and
 * READ as 32-bit words: 4-byte aligned and readable to a multiple of 4 bytes; bits at or past nrows
 * in the last word are ignored.  *out_count (device int64, required) receives the number of rows
 * kept; the host never reads it.  out_offsets needs nrows + 1 entries: entries [0, count] are the
 * scan, entries (count, nrows] repeat out_offsets[count], so any prefix of at least count + 1 entries
 * is a valid offsets array and the buffer's contents are deterministic.  out_indices (optional,
 * nrows entries) receives the source row numbers kept in [0, count) and -1 in [count, nrows): use it
 * to gather side columns.  Capacity and the measure form as for take.  is_fixed schemas: row_offsets
 * and out_offsets may be NULL (out_offsets[j], when given, = min(j, count) * fixed_size); the count
 * is not known on the host, so out_rows != NULL with out_capacity < nrows * fixed_size returns
 * FURY_ERR_CAPACITY before any device work (out_rows == NULL: no capacity check).
 *
 * Bounds (both calls): a source row i is copied only when i is in [0, nrows), its extent
 * [row_offsets[i], row_offsets[i + 1]) lies inside [0, row_offsets[nrows]), and the extent starts at a
 * multiple of 8 with a non-negative size that is a multiple of 8.  Otherwise the output row has size
 * 0 (is_fixed schemas, where only the index can fail: its fixed_size bytes are written as zeros) and
 * FURY_ERR_OUT_OF_BOUNDS is reported on `stream` (fury_device_status), naming the output position j
 * for take and the source row for filter.  Nothing outside the source batch is read and nothing
 * outside [out_rows, out_rows + min(out_capacity, bytes needed)) is written.
 * `rows` and `out_rows` are 8-byte aligned and must not overlap: overlapping buffers give unspecified
 * contents, never an access outside the two buffers.  num_selected == 0 (take) / nrows == 0 (filter)
 * still writes out_offsets[0] = 0 (when given) and *out_count = 0.  Both calls are asynchronous on
 * `stream` with no host synchronisation; argument errors are returned before any device work. */
int fury_row_take(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                  int64_t nrows, const int64_t* indices, int64_t num_selected,
                  void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);
int fury_row_filter(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, const uint8_t* row_mask,
                    void* out_rows, int64_t out_capacity, int64_t* out_offsets,
                    int64_t* out_count, int64_t* out_indices, void* stream);

/* Rows by key, batches end to end -- BinaryRow.copy() over a batch again (FMT/row/binary/
 * BinaryRow.java:173-179): a row is its bytes, unchanged, at a new position, so `schema` may be
 * anything the library creates (flat, wide, nested, a collection schema).
 *
 * fury_row_partition: fury_row_filter from 2 ways to num_parts ways, 1 <= num_parts <=
 * FURY_PARTITION_MAX_PARTS (the ids and one drop bucket fit 16 bits).  part_ids is device int32 with
 * nrows entries.  Row i is KEPT when 0 <= part_ids[i] < num_parts; any other value, negative or too
 * large, DROPS the row as a 0 mask bit does in filter, and a dropped row's extent is never examined.
 * The kept rows come out sorted by (partition id, source row number) -- a stable partition -- so each
 * partition's rows are contiguous and in source order; count = the number of kept rows.
 *   out_part_rows  (device int64, num_parts + 1 entries, required) out_part_rows[p] = the number of
 *                  kept rows with id < p, out_part_rows[num_parts] = count.  Partition p is output
 *                  rows [out_part_rows[p], out_part_rows[p + 1]), its bytes are
 *                  [out_offsets[out_part_rows[p]], out_offsets[out_part_rows[p + 1]]).  The host never
 *                  reads it.
 *   out_offsets    nrows + 1 entries: [0, count] are the scan of the kept rows' sizes in output order,
 *                  (count, nrows] repeat out_offsets[count], exactly as filter does.
 *   out_indices    (optional, nrows entries) the source row of output position j < count, -1 at or
 *                  past the count.
 *   out_positions  (optional, nrows entries) the output position of source row i, -1 for a dropped
 *                  row: the inverse permutation.  fury_row_take of the partitioned batch at the
 *                  positions of the kept rows restores source order.
 * Every entry of every output array is written exactly once per call: the buffers are deterministic.
 * Capacity, the measure form (out_rows == NULL), alignment, the no-overlap rule and the "batch too
 * large" limit are those of fury_row_filter.  is_fixed schemas follow filter's rules too: row_offsets
 * is ignored and may be NULL, out_offsets may be NULL (when given, out_offsets[j] = min(j, count) *
 * fixed_size), and out_rows != NULL with out_capacity < nrows * fixed_size returns FURY_ERR_CAPACITY
 * before any device work.  Bounds: a kept source row whose extent fails the rule of fury_row_take /
 * fury_row_filter has size 0 -- it still occupies its output position -- and raises
 * FURY_ERR_OUT_OF_BOUNDS on `stream`, naming that source row.  nrows == 0: out_part_rows is all zeros
 * and out_offsets[0] = 0 (when given).  Asynchronous on `stream` with no host synchronisation.
 * Argument errors are returned before any device work, a pending device error of `stream` after them
 * and before the call's own work.
 * Consequences: (a) the output equals fury_row_take with the stable argsort of the kept ids;
 * (b) with num_parts == 1 and part_ids[i] = mask_bit(i) - 1, out_rows, out_offsets, out_part_rows[1]
 * and out_indices equal fury_row_filter's out_rows, out_offsets, *out_count and out_indices byte for
 * byte.
 *
 * fury_row_concat: glues 1 <= num_sources <= FURY_CONCAT_MAX_SOURCES batches of `schema` end to end,
 * the vertical counterpart of fury_row_zip.  With N = the sum of the sources' nrows and R_k = the sum
 * over the sources before source k, output row R_k + i is the bytes of row i of source k; out_offsets
 * has N + 1 entries.  A source's row_offsets[0] need not be 0 (an interior slice of a larger batch
 * with its offsets as they are).  Each source row obeys take's extent rule against ITS OWN source's
 * [0, row_offsets_k[nrows_k]); a failing row has size 0 (is_fixed schemas: cannot fail) and raises
 * FURY_ERR_OUT_OF_BOUNDS naming the output position.  Sources may alias each other; out_rows overlaps
 * none of them.  Capacity, the measure form, the is_fixed form (out_offsets optional, FURY_ERR_CAPACITY
 * up front when out_capacity < N * fixed_size) and N == 0 follow fury_row_take.  No host
 * synchronisation: the sources' byte totals stay on the device.  Argument errors are returned before
 * any device work.
 * Consequences: concat of the num_parts slices of a partitioned batch, in partition order, returns
 * the partitioned batch's first count rows byte for byte; concat of one source equals fury_row_take
 * with indices 0, 1, ..., nrows - 1. */
#define FURY_PARTITION_MAX_PARTS 65535
int fury_row_partition(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, const int32_t* part_ids, int32_t num_parts,
                       void* out_rows, int64_t out_capacity, int64_t* out_offsets,
                       int64_t* out_part_rows, int64_t* out_indices, int64_t* out_positions,
                       void* stream);
#define FURY_CONCAT_MAX_SOURCES 32
typedef struct fury_concat_source {
  const void* rows;            /* device, 8-byte aligned; may be NULL when nrows == 0 */
  const int64_t* row_offsets;  /* nrows + 1 entries; ignored (may be NULL) when schema is_fixed */
  int64_t nrows;
} fury_concat_source;
int fury_row_concat(const fury_schema* schema, const fury_concat_source* sources, int32_t num_sources,
                    void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* Key hash -- the batch form of reading a row's key fields with BinaryRow's getters and feeding them
 * to MurmurHash3.murmurhash3_x86_32 (fury-core util/MurmurHash3.java; the same function is in
 * cpp/fury/thirdparty/MurmurHash3.cc): a 32-bit hash and a partition id per row, the ids
 * fury_row_partition takes.  The definition is normative, so that a worker in any language routes a
 * lookup key to the partition the device chose:
 *   1. H(bytes, seed) is MurmurHash3_x86_32 over a byte string: h = seed; every whole 4-byte block,
 *      read little-endian as k, gives k *= 0xcc9e2d51, k = rotl32(k, 15), k *= 0x1b873593, h ^= k,
 *      h = rotl32(h, 13), h = h * 5 + 0xe6546b64; the 1-3 bytes left over, little-endian and
 *      zero-extended as k, give k *= 0xcc9e2d51, k = rotl32(k, 15), k *= 0x1b873593, h ^= k; the
 *      result is fmix32(h ^ len), fmix32(h): h ^= h >> 16, h *= 0x85ebca6b, h ^= h >> 13,
 *      h *= 0xc2b2ae35, h ^= h >> 16.  All arithmetic is modulo 2^32.  Bit-identical to the
 *      reference's murmurhash3_x86_32(byte[] data, int offset, int len, int seed).
 *   2. For row r and the key fields fields[0 .. num_keys) IN THE GIVEN ORDER: h = seed; for each key
 *      k, h = fmix32(h ^ 0xFFFFFFFF) when the field is null in row r, else h = H(value_bytes(k, r), h)
 *      -- each value's hash seeds the next.  A null is a zero-length value whose length word is
 *      0xFFFFFFFF, so null and the empty string differ.  hash[r] = h.
 *   3. value_bytes are the bytes of the column value fury_row_project produces for the field.
 *      BOOL: one byte, 0 or 1.  INT8 / INT16 / INT32 / FLOAT32 / DATE32 / INT64 / FLOAT64 / TIMESTAMP:
 *      the value little-endian at its width (1 / 2 / 4 / 4 / 4 / 8 / 8 / 8 bytes).  Floats are hashed
 *      as their raw bits: -0.0 and 0.0 hash differently, and so do NaNs of different payloads.
 *      DECIMAL: the 16 value bytes.  STRING / BINARY: the payload bytes, of any length (none for the
 *      empty string).
 *   4. part_id[r] = (int32)(hash[r] % (uint32)num_parts), hash[r] taken as unsigned.
 *   5. A LIST, STRUCT or MAP key returns FURY_ERR_UNSUPPORTED: their stored bytes are not canonical
 *      (null slots keep stale contents), so equal values need not have equal bytes.
 * fury_row_hash: 1 <= num_keys <= 64; the checks on `schema` and `fields` and their error codes are
 * fury_row_project's (a collection schema or more than 64 keys FURY_ERR_UNSUPPORTED; num_keys <= 0, an
 * index that is not a field, a field given twice FURY_ERR_INVALID_ARGUMENT).  out_hashes (device
 * uint32, nrows entries) and out_part_ids (device int32, nrows entries) are each optional, but not
 * both NULL; num_parts is used only when out_part_ids is given and must then be in [1, INT32_MAX].
 * `rows` is device memory, 8-byte aligned; row_offsets is ignored and may be NULL for an is_fixed
 * schema (row i at i * fixed_size), as in fury_row_take.  nrows == 0 does nothing.  The call is
 * asynchronous on `stream`, never synchronises with the host and allocates no workspace.
 * Bounds are those of fury_row_project: a row whose header leaves [0, row_offsets[nrows]) has every
 * key null, a key value whose bytes leave it (or whose size is negative) is null, and both raise
 * FURY_ERR_OUT_OF_BOUNDS on `stream` naming the row; the hash and id of such a row follow rule 2 with
 * those nulls, so every entry of the given outputs is always written.  Nothing outside the batch is
 * read, and a corrupt slot of a field that is not a key is never seen.
 * Consequence: fury_row_hash equals rules 1-4 applied to the columns fury_row_project decodes for the
 * same fields.
 * Limits: MurmurHash3's chain is serial within a value, so one value is hashed by one lane however
 * long it is; keys of several KB per row run at that lane's rate.
 *
 * fury_hash_bytes / fury_hash_null (host, no device work): H(bytes[0, len), seed) of rule 1 and
 * fmix32(seed ^ 0xFFFFFFFF) of rule 2, for a CPU worker that routes a key the same way: chain them
 * over the key's values as rule 2 does.  0 <= len <= INT32_MAX (bytes may be NULL when len == 0);
 * otherwise fury_hash_bytes returns 0 and fury_last_error says why. */
int fury_row_hash(const fury_schema* schema, const int32_t* fields, int32_t num_keys,
                  const void* rows, const int64_t* row_offsets, int64_t nrows,
                  uint32_t seed, int32_t num_parts,
                  uint32_t* out_hashes, int32_t* out_part_ids, void* stream);
uint32_t fury_hash_bytes(const void* bytes, int64_t len, uint32_t seed);
uint32_t fury_hash_null(uint32_t seed);

/* Key equality -- the verify step of an equi-join, a group-by or a de-duplication: do the key fields
 * of row i of one batch equal the key fields of row j of another?  The batch form of reading both
 * rows' key fields with BinaryRow's getters and comparing the values, answered from the row bytes with
 * nothing decoded.  fury_row_hash finds candidates (a 32-bit hash collides); this call decides them.
 * The definition is normative, so that a worker in any language agrees with the device:
 *   1. Pairs.  Pair j compares row L = left.indices[j] (left.indices == NULL: L = j) of the left batch
 *      with row R = right.indices[j] (or j) of the right batch, key position by key position:
 *      left.fields[k] is compared with right.fields[k], 0 <= k < num_keys.
 *   2. Key positions.  Both fields null: equal iff FURY_KEYS_NULL_EQUAL is set in `flags`.  Exactly
 *      one null: not equal.  Neither null: equal iff their value_bytes have the same length and the
 *      same bytes, value_bytes being rule 3 of fury_row_hash (the bytes fury_row_project would produce
 *      for the field).  BOOL is one byte, 0 or 1: any non-zero stored byte is 1.  Floats compare as
 *      their raw bits: -0.0 != 0.0, and two NaNs are equal iff their payloads are.  Padding bytes after
 *      a payload are never compared.
 *   3. Outputs.  out_equal[j] (device uint8, num_pairs entries) = 1 iff every key position is equal,
 *      else 0.  Bit j of out_mask (device uint32 words, word j / 32, LSB first: the convention of
 *      fury_row_filter's row_mask) is the same value; all (num_pairs + 31) / 32 words are written
 *      whole, the bits at or past num_pairs zero.  Either output may be NULL, not both.
 *   4. Consequence.  With FURY_KEYS_NULL_EQUAL, a pair that is equal has equal fury_row_hash values on
 *      both sides (each side hashed over its own key fields, in key order) for any seed: unequal
 *      hashes prove inequality.
 *   5. Bounds are the "Decode bounds" as fury_row_hash applies them, per side, against that side's own
 *      [0, row_offsets[nrows]) (is_fixed: [0, nrows * fixed_size)).  A failure is an index outside
 *      [0, nrows), a row whose header leaves the batch, a key value whose span leaves the batch, or a
 *      key value whose size is negative.  Any failure makes the pair NOT EQUAL WHATEVER THE FLAGS and
 *      raises FURY_ERR_OUT_OF_BOUNDS on `stream` (fury_device_status), naming the pair number j as
 *      fury_row_take names its output row.  All keys of a pair are always examined for null bits and
 *      bounds, so whether an error is raised does not depend on an earlier key having differed;
 *      payload bytes are read only where both values are non-null, in bounds and of equal length.
 *      Nothing outside either batch is read, and slots of fields that are not keys are never looked
 *      at.
 *   6. Key types are those of fury_row_hash: a LIST, STRUCT or MAP key returns FURY_ERR_UNSUPPORTED,
 *      for the reason of hash rule 5.  left.fields[k] and right.fields[k] must have the same type_id,
 *      else FURY_ERR_INVALID_ARGUMENT naming k and both fields.  The two schemas may differ in every
 *      other way: other fields, the key fields' slot positions, fixed-size against variable-length
 *      rows.
 * 1 <= num_keys <= 64; the checks on each side's `schema` and `fields` and their error codes are
 * fury_row_hash's.  num_pairs and each nrows are >= 0; a side without `indices` needs nrows >=
 * num_pairs.  `rows` (device, 8-byte aligned), row_offsets and indices (device, 8-byte aligned) follow
 * fury_row_take; out_mask is 4-byte aligned.  Unknown bits in `flags` return
 * FURY_ERR_INVALID_ARGUMENT.  num_pairs == 0 does nothing and returns FURY_OK.  The call is
 * asynchronous on `stream`, never synchronises with the host and allocates no workspace.
 * Limits: a value is compared by one lane however long it is; keys of several KB per row run at that
 * lane's rate. */
typedef struct fury_key_side {
  const fury_schema* schema;
  const int32_t* fields;        /* num_keys key fields, in key order (host) */
  const void* rows;             /* device, 8-byte aligned */
  const int64_t* row_offsets;   /* device; ignored for an is_fixed schema, as in fury_row_hash */
  int64_t nrows;
  const int64_t* indices;       /* device, num_pairs entries; NULL: pair j uses row j */
} fury_key_side;
#define FURY_KEYS_NULL_EQUAL 1  /* two null keys compare equal (group-by); default: they do not (SQL join) */
int fury_row_keys_equal(const fury_key_side* left, const fury_key_side* right, int32_t num_keys,
                        int64_t num_pairs, int32_t flags,
                        uint8_t* out_equal, uint32_t* out_mask, void* stream);

/* Group ids and distinct rows -- the batch form of reading every row's key fields with BinaryRow's
 * getters and putting the rows into a LinkedHashMap keyed by the values: which rows of ONE batch have
 * equal keys, answered from the row bytes with nothing decoded and in time linear in nrows (the
 * self-join through fury_row_keys_equal is quadratic in the size of a group).  The definition is
 * normative; the output is a pure function of the batch and the key fields:
 *   1. Groups.  Two rows are in the same group iff every key position is equal under rule 2 of
 *      fury_row_keys_equal with FURY_KEYS_NULL_EQUAL: null equals null, null differs from the empty
 *      string, floats compare as their raw bits (-0.0 != 0.0, NaNs by payload), BOOL is 0 or 1 (any
 *      non-zero stored byte is 1), padding bytes after a payload are never compared.
 *   2. First rows.  out_first[i] (device int64, nrows entries, required) = the smallest row number in
 *      row i's group.  It is deterministic: independent of how the device schedules the rows.
 *   3. Numbering.  Groups are numbered in the order of their first rows; G = the number of groups.
 *      out_group_ids[i]  (optional, nrows entries) = the number of groups whose first row is less than
 *                        out_first[i]: in [0, G).
 *      out_group_rows[g] (optional, nrows entries) = the first row of group g for g < G, -1 for
 *                        G <= g < nrows.
 *      *out_num_groups   (optional, 1 entry) = G.
 *      Every entry of every given output is written exactly once per call.
 *      Consequences: (a) fury_row_take at out_group_rows[0 .. G) returns the distinct rows in source
 *      order (de-duplication keeps the first occurrence); (b) out_group_ids, narrowed to int32, fed to
 *      fury_row_partition with num_parts = G (G <= FURY_PARTITION_MAX_PARTS) makes every group
 *      contiguous, groups in order of first occurrence, rows in source order; (c) out_first[i] ==
 *      out_group_rows[out_group_ids[i]].
 *   4. Hashes.  hashes == NULL: the call hashes the keys itself, as fury_row_hash does with seed 0,
 *      into workspace.  hashes != NULL (device uint32, nrows entries): any function of the key values
 *      will do -- rows with equal keys must have equal entries -- for example the out_hashes of
 *      fury_row_hash over the same keys with any seed, so a shuffle's hashes are not computed twice.
 *      The hash only chooses where probing starts and which rows are compared; correctness never
 *      rests on its quality (all-equal hashes give the same outputs, slowly).  If the caller breaks
 *      the condition, rows with equal keys may land in different groups; nothing else may happen: no
 *      read outside the batch, every output is still written, out_first[i] <= i and the numbering of
 *      rule 3 holds for the groups that were formed.
 *   5. Bounds are the "Decode bounds" as fury_row_hash applies them.  A row whose header leaves
 *      [0, row_offsets[nrows]) (is_fixed: [0, nrows * fixed_size)), or a key value whose span leaves
 *      it or whose size is negative, makes row i a group of its own (out_first[i] = i); the row is
 *      never entered into the table and never compared with another row, and it raises
 *      FURY_ERR_OUT_OF_BOUNDS on `stream` (fury_device_status) naming row i.  Nothing outside the
 *      batch is read, and slots of fields that are not keys are never looked at.
 *   6. Key types and the checks on `schema`, `fields` and `num_keys`, with their error codes, are those
 *      of fury_row_hash: 1 <= num_keys <= 64, a LIST, STRUCT or MAP key returns FURY_ERR_UNSUPPORTED.
 * out_first == NULL returns FURY_ERR_INVALID_ARGUMENT.  `rows`, row_offsets and the int64 outputs are
 * device memory, 8-byte aligned, `hashes` 4-byte aligned; row_offsets is ignored and may be NULL for an
 * is_fixed schema, as in fury_row_hash.  nrows == 0 writes *out_num_groups = 0 when it is given and
 * nothing else.  nrows > 2^31 - 1 returns FURY_ERR_INVALID_ARGUMENT ("batch too large").  The call is
 * asynchronous on `stream` and never synchronises with the host; argument errors are returned before
 * any device work.
 * Workspace (stream-ordered, freed on `stream`): one 8-byte table slot for each of the smallest power
 * of two >= 2 * nrows slots (16 to 32 bytes per row), 4 bytes per row of slot indices, 4 bytes per row
 * of hashes when hashes == NULL, and 8 bytes per row (plus nrows / 255 words of scan scratch) when any
 * output but out_first is given: at most 48 bytes per row.
 * Limits: a value is compared by one lane however long it is, as in fury_row_keys_equal. */
int fury_row_group(const fury_schema* schema, const int32_t* fields, int32_t num_keys,
                   const void* rows, const int64_t* row_offsets, int64_t nrows,
                   const uint32_t* hashes,      /* device, nrows entries, optional */
                   int64_t* out_first,          /* device, nrows entries, required */
                   int64_t* out_group_ids,      /* device, nrows entries, optional */
                   int64_t* out_group_rows,     /* device, nrows entries, optional */
                   int64_t* out_num_groups,     /* device, 1 entry, optional */
                   void* stream);

/* Key index and lookup -- the probe side of a hash join: for every row of a probe batch, is its key
 * present in a build batch, and at which row?  The batch form of HashMap.putIfAbsent(key fields, row)
 * over the build batch (fury_row_index_build) followed by HashMap.get(key fields) for every probe row
 * (fury_row_lookup), the key fields read with BinaryRow's getters, answered from the row bytes with
 * nothing decoded.  One index serves any number of lookups: a dimension join, a semi-join or anti-join
 * (IN / NOT IN), an upsert, a build side probed by a stream of batches.  The definition is normative;
 * every output is a pure function of the two batches, the key fields and the flags:
 *   1. Slots.  fury_row_index_slots(nrows) (host, no device work) = the smallest power of two that is at
 *      least max(2, 2 * nrows): the number of 8-byte words of the table of a build batch of nrows rows.
 *      It returns -1 for nrows < 0 or nrows > 2^31 - 1.
 *   2. Build.  fury_row_index_build enters the rows of one batch into `table` (device, the caller's
 *      memory, 8-byte aligned, required; table_slots words) exactly as fury_row_group builds its own
 *      table: the same kernel, the equality of rule 1 of fury_row_group (null equals null), its rule 4
 *      for `hashes` and its rule 5 for bounds.  A row that fails the bounds is never entered and raises
 *      FURY_ERR_OUT_OF_BOUNDS on `stream` naming the row.  table_slots must equal
 *      fury_row_index_slots(nrows), else FURY_ERR_INVALID_ARGUMENT.  out_first (device int64, nrows
 *      entries, optional) receives what fury_row_group's out_first receives: the smallest row of row
 *      i's group, its own number for a row that was not entered.  nrows == 0 marks the table's two
 *      slots empty and writes nothing else.  Key types and the checks on `schema`, `fields` and
 *      `num_keys` are those of fury_row_group (its rule 6); nrows > 2^31 - 1 is "batch too large".
 *   3. The table.  Its contents are opaque: one slot per distinct key, holding the smallest entered row
 *      of that key once the build has completed, but which slot a key lives in depends on how the
 *      device scheduled the rows.  It is valid for lookups only with THIS batch, unmodified, THESE key
 *      fields, the same hash function, and after the build has completed on its stream (a lookup on
 *      the same stream is ordered behind it).
 *   4. Lookup.  For probe row j, out_rows[j] (device int64, probe->nrows entries) = the smallest row i
 *      of `build` that was entered into the table and whose key fields equal those of probe row j, or
 *      -1 if there is none.  Equality is rule 2 of fury_row_keys_equal under `flags`
 *      (FURY_KEYS_NULL_EQUAL or 0), probe->fields[k] compared with build->fields[k].  Bit j of
 *      out_mask (device uint32 words, word j / 32, LSB first: the convention of fury_row_filter's
 *      row_mask) = (out_rows[j] >= 0); all (probe->nrows + 31) / 32 words are written whole, the bits
 *      at or past probe->nrows zero.  Either output may be NULL, not both.  With flags == 0 a probe
 *      row with a null key matches nothing: it gets -1 without the table being walked, after its
 *      bounds have been examined.  `indices` must be NULL on both sides (the call takes whole batches),
 *      else FURY_ERR_INVALID_ARGUMENT.
 *   5. Hashes.  probe_hashes == NULL: the call hashes the probe keys itself, as fury_row_hash does
 *      with seed 0, into workspace; this pairs with a build whose `hashes` was NULL.  Otherwise
 *      (device uint32, probe->nrows entries) the caller passes the same function of the key values
 *      that the build got.  The hash only chooses where the walk starts and which slots are compared:
 *      a mismatch between the two sides can only turn a match into -1, never produce a wrong match.
 *   6. Probe-side bounds follow rule 5 of fury_row_keys_equal: a probe row whose header or key value
 *      leaves its batch (or whose key size is negative) gets -1 and mask bit 0 whatever the flags, and
 *      raises FURY_ERR_OUT_OF_BOUNDS on `stream` naming j.  Slots of fields that are not keys are never
 *      looked at.
 *   7. Table robustness.  The table is the caller's memory, so the lookup trusts none of it.  A slot on
 *      row j's walk whose hash half equals j's hash and whose row half is >= build->nrows gives -1 for
 *      j and raises FURY_ERR_OUT_OF_BOUNDS naming j; so does a named build row whose header or key
 *      value leaves the build batch: the row is checked before any of its payload is read.  The walk
 *      ends after at most table_slots steps, with -1.  For ANY table contents out_rows[j] is -1 or a
 *      build row whose keys really equal those of probe row j, and nothing outside either batch or
 *      the table's table_slots words is read.
 *   8. Key types.  The two schemas need to share only the key types: rule 6 of fury_row_keys_equal,
 *      same checks and messages (with "probe" and "build" for "left" and "right").
 * fury_row_lookup: 1 <= num_keys <= 64.  `table` is required, 8-byte aligned, and table_slots must
 * equal fury_row_index_slots(build->nrows), else FURY_ERR_INVALID_ARGUMENT; out_rows is 8-byte, out_mask
 * and probe_hashes 4-byte aligned; `rows` and row_offsets follow fury_row_keys_equal.  A build batch of
 * no rows may have rows == NULL and row_offsets == NULL: every probe row gets -1.  Unknown bits in
 * `flags` return FURY_ERR_INVALID_ARGUMENT.  probe->nrows == 0 does nothing and returns FURY_OK.  Both calls are
 * asynchronous on `stream` and never synchronise with the host; argument errors are returned before
 * any device work.
 * Workspace (stream-ordered, freed on `stream`): build: 4 bytes per row when the call hashes itself,
 * plus 4 bytes per row when out_first is given; lookup: 4 bytes per probe row when the call hashes
 * itself, else none.
 * Limits: device memory only; at most 2^31 - 1 build rows; a value is compared by one lane however
 * long it is, as in fury_row_keys_equal. */
int64_t fury_row_index_slots(int64_t nrows);
int fury_row_index_build(const fury_schema* schema, const int32_t* fields, int32_t num_keys,
                         const void* rows, const int64_t* row_offsets, int64_t nrows,
                         const uint32_t* hashes,      /* device, nrows entries, optional */
                         uint64_t* table,             /* device, table_slots words, the caller's memory */
                         int64_t table_slots,         /* fury_row_index_slots(nrows) */
                         int64_t* out_first,          /* device, nrows entries, optional */
                         void* stream);
int fury_row_lookup(const fury_key_side* probe, const fury_key_side* build, int32_t num_keys,
                    const uint64_t* table, int64_t table_slots,
                    const uint32_t* probe_hashes,     /* device, probe->nrows entries, optional */
                    int32_t flags,                    /* FURY_KEYS_NULL_EQUAL */
                    int64_t* out_rows,                /* device, probe->nrows entries */
                    uint32_t* out_mask,               /* device, (probe->nrows + 31) / 32 words */
                    void* stream);

/* The order of rows -- ORDER BY, top-k, a sortedness check, a binary search (range partitioning, merge
 * joins), sorted runs: which of two rows' key fields is smaller?  The batch form of reading both rows'
 * key fields with BinaryRow's getters and comparing the values key after key, answered from the row
 * bytes with nothing decoded.  The reference ships no comparator of rows; the order below is this
 * library's and is normative, so that a worker in any language orders rows as the device does:
 *   1. Keys.  Pair j is pair j of fury_row_keys_equal (rule 1 there: rows left.indices[j] / right.indices[j],
 *      or row j).  The rows are compared key position by key position, left.fields[k] against
 *      right.fields[k]; the first position that differs decides, and the result is -1 (the left row
 *      sorts first), 0 or +1.
 *   2. Nulls.  Null against null is equal.  Null against a value: the null is smaller, or greater when
 *      the position has FURY_ORDER_NULLS_LAST.  The placement is absolute: FURY_ORDER_DESC does not
 *      flip it.
 *   3. Value order, ascending.  BOOL: false < true, any non-zero stored byte being true.  INT8 / INT16 /
 *      INT32 / INT64 / DATE32 / TIMESTAMP: signed at their width (a slot is zero-extended, so the sign
 *      is taken at the width).  FLOAT32 / FLOAT64: IEEE-754 totalOrder of the raw bits: negative NaNs <
 *      -inf < ... < -0.0 < +0.0 < ... < +inf < positive NaNs, NaNs ordered by payload.  This is not
 *      Double.compare, which collapses the NaNs; it is chosen so that rule 5 holds.  DECIMAL: the 16
 *      value bytes as a signed little-endian 128-bit integer (what Arrow's decimal128 and
 *      BinaryWriter.writeDecimal store); the schema carries no scale, so equal scales are the
 *      caller's business.  STRING / BINARY: unsigned byte-wise lexicographic, a proper prefix smaller.
 *      For valid UTF-8 this is Unicode code-point order, NOT String.compareTo's UTF-16 code-unit order:
 *      the two differ for supplementary characters against U+E000..U+FFFF.
 *   4. Direction.  FURY_ORDER_DESC reverses rule 3 for that key position only.
 *   5. Consistency.  For a pair without a bounds failure the result is 0 if and only if
 *      fury_row_keys_equal with FURY_KEYS_NULL_EQUAL says equal: -0.0 and +0.0 differ, two NaNs are
 *      equal iff their bits are, null differs from the empty string.
 *   6. Bounds are the "Decode bounds" as fury_row_hash applies them, per side against that side's own
 *      batch.  An index outside [0, nrows) or a row whose header leaves the batch makes every key of
 *      that row null; a key value whose span leaves the batch or whose size is negative is null.  Each
 *      such failure raises FURY_ERR_OUT_OF_BOUNDS on `stream` (fury_device_status) naming the pair (or
 *      output) number j.  The result is still defined, by rules 1-4 with those nulls, and still a total
 *      preorder, so a sort of a corrupt batch terminates and is deterministic.  All keys of a pair are
 *      examined for null bits and bounds whatever the earlier keys gave, as in fury_row_keys_equal.
 *      Nothing outside either batch is read, and slots of fields that are not keys are never looked at.
 * Key types, the key count (1..64), the checks on each side's `schema` and `fields`, the equal type_id
 * at every key position and their error codes are fury_row_keys_equal's.  key_flags: a host array of
 * num_keys entries, each a combination of FURY_ORDER_DESC and FURY_ORDER_NULLS_LAST; NULL: all zeros
 * (ascending, nulls first).  Unknown bits return FURY_ERR_INVALID_ARGUMENT.
 *
 * fury_row_compare: out_cmp[j] (device int8, num_pairs entries, required) = -1 / 0 / +1 for pair j.
 * num_pairs == 0 returns FURY_OK and does nothing.  The call is asynchronous on `stream`, never
 * synchronises with the host and allocates no workspace.
 *
 * fury_row_order_words: the piece that lets an integer sort order rows.  NK(value), the normalised key
 * bytes, is a byte string whose unsigned lexicographic order, prefix smaller, is rule 3: a fixed-width
 * value big-endian at its width with the sign bit flipped (floats: a negative value has all bits
 * flipped, any other the sign bit set); BOOL one byte, 0 or 1; DECIMAL 16 bytes big-endian with the
 * sign bit flipped; STRING / BINARY the payload.  Output j describes row indices[j] (indices == NULL:
 * row j, and num_out <= nrows) by one signed 64-bit word for chunk `chunk` >= 0 of key field `field`:
 * the bytes NK[7 chunk, 7 chunk + 7), zero-padded, big-endian in bits 63..8; the low byte 1 + the number
 * of value bytes in the chunk (1..8), or 9 when more bytes follow the chunk; FURY_ORDER_DESC complements
 * all 64 bits of a non-null word; a null, or a value failed under rule 6, is the minimum of the encoding
 * (all bits 0), or the maximum (all bits 1) with FURY_ORDER_NULLS_LAST; finally the top bit is flipped,
 * so that SIGNED int64 comparison of the words is the order.  For rows equal on all earlier chunks of
 * this key: the signed order of the words is the order of rules 2-4; equal words whose low byte says
 * "ended" mean equal values; "more follows" means the next chunk decides.  A chunk past the end of
 * every value yields "ended" words with no value bytes.  *out_more (device uint32, optional) is set to
 * 1 when any output row's value continues past the chunk, else 0.  8-byte keys take two chunks, DECIMAL
 * three.  out_words (device, 8-byte aligned, num_out entries) is required; `flags` are the FURY_ORDER_*
 * bits of this key.  The call is asynchronous on `stream`, never synchronises with the host and
 * allocates no workspace.
 * Limits: device memory only; a value is compared (or its chunk read) by one lane however long it is. */
#define FURY_ORDER_DESC 1        /* this key position descending (nulls stay where rule 2 puts them) */
#define FURY_ORDER_NULLS_LAST 2  /* nulls of this key position sort after every value */
int fury_row_compare(const fury_key_side* left, const fury_key_side* right, int32_t num_keys,
                     const int32_t* key_flags,        /* host, num_keys entries, or NULL */
                     int64_t num_pairs,
                     int8_t* out_cmp,                 /* device, num_pairs entries */
                     void* stream);
int fury_row_order_words(const fury_schema* schema, int32_t field, int32_t flags, int32_t chunk,
                         const void* rows, const int64_t* row_offsets, int64_t nrows,
                         const int64_t* indices,      /* device, num_out entries, or NULL */
                         int64_t num_out,
                         int64_t* out_words,          /* device, num_out entries */
                         uint32_t* out_more,          /* device, one word, optional */
                         void* stream);

/* Per-group aggregates -- the last step of a GROUP BY: COUNT / SUM / MIN / MAX of value fields, and the
 * row that holds the smallest or largest value, for every group of a batch whose rows carry a group id
 * (fury_row_group's out_group_ids).  The batch form of reading every row's value field with BinaryRow's
 * getters and folding it into the accumulator of the row's group, answered from the row bytes in one
 * pass over the row headers, with nothing decoded.  Up to FURY_AGG_MAX_AGGS aggregates share that pass.
 * The definition is normative; but for the float sums of rule 3 every output is a pure function of the
 * batch, the ids and the aggregates:
 *   1. Groups.  Row i belongs to group group_ids[i] (device int64, nrows entries).  A row whose id is
 *      outside [0, num_groups) takes part in nothing and is not an error: fury_row_partition's rule,
 *      and how a WHERE mask is applied (give the rows that fail it the id -1).  group_ids == NULL
 *      requires num_groups == 1 and puts every row in group 0: the aggregates of the whole batch.
 *   2. Values and nulls.  A value is what the projected decode (fury_row_project) produces for that
 *      field of that row.  Nulls never take part.  out_count[g] (optional) = the number of values of
 *      group g that took part in this aggregate.  A group with no values gets out[g] = 0 for COUNT,
 *      SUM, MIN and MAX, and -1 for ARGMIN / ARGMAX: out_count[g] == 0 is the result's null flag.
 *      COUNT looks only at the null bit, so it accepts a field of any type, LIST / STRUCT / MAP
 *      included; with field == -1 it counts every row of the group, COUNT(*).
 *   3. SUM.  INT8 / INT16 / INT32 / INT64: the int64 sum of the sign-extended values with two's
 *      complement wrap-around; exact and independent of order.  FLOAT32 / FLOAT64: a double; every
 *      value is widened exactly and the values are added in double, in an unspecified order, so this
 *      is the only output of the call that may differ between two runs.  Its error against the exact
 *      sum is at most (m - 1) * 2^-52 * sum |x| for m finite values, the bound of any summation order
 *      in double; NaN and infinities propagate as IEEE addition propagates them.  Any other type
 *      returns FURY_ERR_UNSUPPORTED naming the route: DECIMAL sums are out of scope; a BOOL sum is the
 *      COUNT of the field under ids that drop the false rows.
 *   4. MIN / MAX are defined for the fixed-width types (INT8 ... INT64, FLOAT32, FLOAT64, DATE32,
 *      TIMESTAMP) and BOOL.  The order is rule 3 of fury_row_compare, ascending: signed at the value's
 *      width, floats by totalOrder of their bits, BOOL 0 < 1.  out[g] holds the winning value's
 *      bytes: integers, DATE32 and TIMESTAMP sign-extended to int64; BOOL 0 / 1; FLOAT64 its 8 bytes;
 *      FLOAT32 its 4 bytes in the low half, the high half zero.  The result is bit-exact, NaN payloads
 *      and -0.0 included.  STRING / BINARY / DECIMAL return FURY_ERR_UNSUPPORTED naming the route:
 *      ARGMIN / ARGMAX, then fury_row_take at the rows whose count is not zero.
 *   5. ARGMIN / ARGMAX are defined for every key type of fury_row_compare: the fixed-width types, BOOL,
 *      DECIMAL, STRING and BINARY, in the value order of its rule 3.  out[g] (int64) = the smallest row
 *      number among the rows of group g whose value is the minimum (maximum) of the group.  It is
 *      deterministic: independent of how the device schedules the rows.  It is consistent:
 *      fury_row_compare of that row against every row of the group with a non-null value, on this
 *      field, is <= 0 (>= 0).
 *   6. Writes.  Every entry of every given `out` and `out_count` (num_groups entries each) is written
 *      exactly once per call, whatever the ids contain.
 *   7. Bounds are the "Decode bounds" as rule 5 of fury_row_group applies them.  A row whose header
 *      leaves [0, row_offsets[nrows]) takes part in nothing.  A STRING / BINARY / DECIMAL value of an
 *      ARGMIN / ARGMAX aggregate whose span leaves the batch, or whose size is negative, counts as
 *      null for that aggregate.  Either raises FURY_ERR_OUT_OF_BOUNDS on `stream`
 *      (fury_device_status) naming the row.  Nothing outside the batch is read, slots of fields that
 *      no aggregate names are never looked at, and group_ids is read at [0, nrows) only.
 *   8. Argument checks, all on the host before any device work: schema, aggs and nrows >= 0 as the
 *      neighbours; 1 <= num_aggs <= FURY_AGG_MAX_AGGS; 0 <= num_groups <= 2^31 - 1; nrows <= 2^31 - 1
 *      ("batch too large"); every op one of FURY_AGG_*; every field a field of the schema (-1 only
 *      with FURY_AGG_COUNT); the types of rules 3-5; every `out` given; `rows`, row_offsets, group_ids
 *      and every out / out_count 8-byte aligned; no two outputs of one call the same pointer.  A
 *      collection schema returns FURY_ERR_UNSUPPORTED, every other failure FURY_ERR_INVALID_ARGUMENT.
 *      One field may appear under several ops, and in several aggregates.
 * num_groups == 0 writes nothing and returns FURY_OK.  nrows == 0 with num_groups > 0 still applies
 * rule 6 (rows and row_offsets may then be NULL).  row_offsets is ignored and may be NULL for an
 * is_fixed schema.  The call is asynchronous on `stream` and never synchronises with the host.
 * Workspace (stream-ordered, freed on `stream`): 24 bytes per group and aggregate -- an accumulator, a
 * count and a row number -- whatever nrows is.
 * Limits: device memory only; a STRING / BINARY value is compared by one lane however long it is. */
#define FURY_AGG_COUNT  1   /* non-null values of `field`; field == -1: every row of the group (COUNT(*)) */
#define FURY_AGG_SUM    2
#define FURY_AGG_MIN    3
#define FURY_AGG_MAX    4
#define FURY_AGG_ARGMIN 5   /* the row that holds the smallest value */
#define FURY_AGG_ARGMAX 6
#define FURY_AGG_MAX_AGGS 16
typedef struct fury_agg {
  int32_t field;        /* top-level slot of the value field */
  int32_t op;           /* FURY_AGG_* */
  void* out;            /* device, num_groups 8-byte entries, required */
  int64_t* out_count;   /* device, num_groups entries, optional: non-null values that took part */
} fury_agg;
int fury_row_aggregate(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                       int64_t nrows,
                       const int64_t* group_ids,  /* device, nrows entries; NULL: every row is in group 0 */
                       int64_t num_groups,
                       const fury_agg* aggs, int32_t num_aggs, void* stream);
/* Host, no device work: the call combines per workgroup on chip when num_groups * num_aggs is at most
 * this many cells, and with global atomics above it.  The results are the same on both sides; tests use
 * it to stand on both. */
int64_t fury_row_aggregate_lds_cells(void);

/* WHERE masks -- which rows of a batch pass a condition on their fields?  The batch form of reading the
 * named fields of every row with BinaryRow's getters and testing each value against a literal, answered
 * from the row bytes with nothing decoded: one bit per row, in the shape fury_row_filter,
 * fury_row_update and the other mask consumers read.  Up to FURY_PRED_MAX_TERMS tests share one pass
 * over the row headers.  The reference ships no predicate over rows; the definition below is this
 * library's and is normative, so that a worker in any language selects the rows the device does:
 *   1. Shape.  The terms form a conjunction of clauses.  Term t starts a new clause unless it carries
 *      FURY_PRED_OR; with FURY_PRED_OR it is OR-ed into the clause of term t - 1 (term 0 with
 *      FURY_PRED_OR is an argument error).  A row passes when every clause has at least one true term.
 *      BETWEEN is two clauses; a short IN list is EQ terms OR-ed together; a long IN list is a
 *      fury_row_lookup against the list, whose out_mask is chained in through row_mask.
 *   2. Fields and literals.  The supported fields are the key types of fury_row_keys_equal: the
 *      fixed-width types (INT8 / INT16 / INT32 / INT64 / FLOAT32 / FLOAT64 / DATE32 / TIMESTAMP), BOOL,
 *      DECIMAL, STRING and BINARY.  A LIST / STRUCT / MAP field returns FURY_ERR_UNSUPPORTED, under
 *      every op, naming the route: fury_row_project / fury_row_extract, then a test on the decoded
 *      value.  The literal is the value's bytes as the projected decode (fury_row_project) would produce
 *      them: a fixed-width type exactly `width` little-endian bytes; BOOL 1 byte, non-zero = true;
 *      DECIMAL 16 bytes, little-endian two's complement; STRING / BINARY any length, 0 included.  A
 *      wrong literal_len for a fixed-size type is an argument error.  The literal is HOST memory and
 *      is copied during the call.  FURY_PRED_IS_NULL takes no literal (literal_len 0).
 *   3. Comparison ops.  FURY_PRED_EQ / LT / LE / GT / GE are true exactly where fury_row_compare
 *      (ascending; rules 3 and 5 there) of the row's value against a value with the literal's bytes
 *      gives 0 / -1 / <= 0 / +1 / >= 0.  Floats therefore compare by totalOrder of their bits: EQ 0.0
 *      does not match -0.0, EQ of a NaN matches the NaNs with the same bits, and a positive NaN is GT
 *      every number.  Strings compare by unsigned bytes, a proper prefix smaller.  The consequence: a
 *      range predicate selects exactly the rows that fury_row_compare's binary search (search_sorted)
 *      delimits in the batch sorted by that field.
 *   4. Pattern ops, STRING / BINARY only, byte-wise on the payload (no code points, no case folding).
 *      FURY_PRED_STARTS_WITH / FURY_PRED_ENDS_WITH: the value has at least literal_len bytes and its
 *      first / last literal_len bytes equal the literal.  FURY_PRED_CONTAINS: the literal occurs at
 *      some byte offset of the value.  An empty literal matches every non-null value.  A pattern op on
 *      any other field returns FURY_ERR_UNSUPPORTED.
 *   5. Nulls.  FURY_PRED_IS_NULL is true where the field's null bit is set; with FURY_PRED_NOT it is
 *      true where the bit is clear.  Every other term on a null value is not true, with or without
 *      FURY_PRED_NOT: FURY_PRED_NOT makes a term true where its test is false and the value is not
 *      null.  Negation exists only on terms and a row must be TRUE to pass, so this is exactly SQL's
 *      three-valued WHERE: a comparison with NULL is UNKNOWN, NOT UNKNOWN is UNKNOWN, and UNKNOWN
 *      does not pass.
 *   6. Outputs.  Bit i of out_mask, LSB-first in 32-bit words (word i / 32, bit i % 32: the shape
 *      fury_row_filter reads), is 1 when row i passes.  Every word in [0, (nrows + 31) / 32) is
 *      written, bits at or past nrows are 0, and nothing past the last word is written.  *out_count,
 *      when given, receives the exact number of set bits.  row_mask, when given, is read in the same
 *      format: a row whose bit is 0 is not read at all and fails.  row_mask == out_mask, the identical
 *      pointer, is allowed and refines a mask in place; any other overlap gives unspecified contents.
 *      nrows == 0 writes *out_count = 0 and touches nothing else.
 *   7. Bounds are rule 6 of fury_row_compare applied to one side.  A row whose header leaves
 *      [0, row_offsets[nrows]) has every field null; a STRING / BINARY / DECIMAL value whose span
 *      leaves the batch, or whose size is negative, is null.  Each such failure raises
 *      FURY_ERR_OUT_OF_BOUNDS on `stream` (fury_device_status) naming the row; the mask is still
 *      defined, by rules 1-5 with those nulls.  Every term's null bit and span are examined whatever
 *      the earlier terms gave, so the reported error does not depend on short-circuiting.  Nothing
 *      outside the batch is read -- this includes the 1-7 bytes that follow the batch's last value --
 *      and slots of fields that no term names are never looked at.
 *   8. Argument checks, all on the host before any device work, every message starting with
 *      fury_row_predicate: schema, terms and out_mask given, nrows >= 0; 1 <= num_terms <=
 *      FURY_PRED_MAX_TERMS; every op one of FURY_PRED_*; no flag bits but FURY_PRED_NOT and
 *      FURY_PRED_OR, no FURY_PRED_OR on term 0; `reserved` 0; every field a field of the schema, of a
 *      type rules 2 and 4 accept; literal_len >= 0, the length rule 2 fixes, 0 for FURY_PRED_IS_NULL;
 *      `literal` not NULL where literal_len > 0; the literal pool -- the sum over the terms of
 *      literal_len rounded up to a multiple of 8 -- at most FURY_PRED_MAX_LITERAL_BYTES; `rows`,
 *      row_offsets and out_count 8-byte aligned, row_mask and out_mask 4-byte aligned; nrows small
 *      enough for one launch ("batch too large" past 2^39 - 256).  A collection schema and the type
 *      failures return FURY_ERR_UNSUPPORTED, every other failure FURY_ERR_INVALID_ARGUMENT.  One field
 *      may appear in several terms.  row_offsets is ignored and may be NULL for an is_fixed schema, as
 *      elsewhere.
 * The call is asynchronous on `stream`, never synchronises with the host and allocates no workspace
 * (out_count is zeroed by a memset on the stream); it is safe to bind and re-issue.
 * Limits: device memory only; a STRING / BINARY value is compared or scanned by one lane however long
 * it is.  FURY_PRED_CONTAINS is the plain search: one comparison of up to 8 bytes per byte offset of
 * the value, and at every offset where the literal's first 8 bytes match, a comparison of the rest of
 * the literal, so its worst case (a repetitive literal of m bytes in a repetitive value of n bytes) is
 * n * m / 8 word comparisons and loads in one lane. */
#define FURY_PRED_IS_NULL      1   /* no literal */
#define FURY_PRED_EQ           2
#define FURY_PRED_LT           3
#define FURY_PRED_LE           4
#define FURY_PRED_GT           5
#define FURY_PRED_GE           6
#define FURY_PRED_STARTS_WITH  7   /* STRING / BINARY only */
#define FURY_PRED_ENDS_WITH    8
#define FURY_PRED_CONTAINS     9
#define FURY_PRED_NOT 1            /* flags: the term is true where the test is false (value non-null) */
#define FURY_PRED_OR  2            /* flags: this term joins the clause of the term before it */
#define FURY_PRED_MAX_TERMS 32
#define FURY_PRED_MAX_LITERAL_BYTES 2048   /* sum over terms of literal_len rounded up to 8 */
typedef struct fury_pred_term {
  int32_t field;            /* top-level slot of the field */
  int32_t op;               /* FURY_PRED_* */
  int32_t flags;            /* FURY_PRED_NOT | FURY_PRED_OR */
  int32_t reserved;         /* must be 0 */
  const void* literal;      /* HOST memory, copied during the call; NULL for FURY_PRED_IS_NULL */
  int64_t literal_len;
} fury_pred_term;           /* 32 bytes */
int fury_row_predicate(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                       int64_t nrows, const fury_pred_term* terms, int32_t num_terms,
                       const uint32_t* row_mask,   /* device, optional: rows to examine */
                       uint32_t* out_mask,         /* device, (nrows + 31) / 32 words, required */
                       int64_t* out_count,         /* device, optional: number of bits set */
                       void* stream);

/* Nested values as batches -- BinaryRow.getStruct / getArray / getMap (ordinal) over a batch
 * (FMT/row/binary/UnsafeTrait.java:160-197; BinaryMap.pointTo, FMT/row/binary/BinaryMap.java:62-77):
 * one bitmap bit, one 8-byte slot and a pointTo(buffer, baseOffset + relativeOffset, size).  A nested
 * row, array or map addresses its variable-length section relative to its own base, so the bytes the
 * slot points at are, unchanged, a complete row of the child schema / a complete top-level
 * BinaryArray (what ArrayEncoder.toArray writes) / a complete BinaryMap [int64 keyArrayBytes][keys]
 * [values] (what MapEncoder.toMap writes).  fury_row_extract packs that value of every row into a new
 * batch, which every other entry point takes with the schema fury_schema_child returns:
 * a.b.name of a bean is extract {a, b} followed by fury_row_project of name.
 *
 * Path (both functions, same rules, each message prefixed with the function's name): path[0] is a
 * top-level slot of `schema`, path[k] a slot of the STRUCT reached by path[0..k); every node but the
 * last is a STRUCT, the last a STRUCT, LIST or MAP; 1 <= path_len <= 64 (the schema depth limit).
 * A null path, path_len out of range or a slot index out of range returns FURY_ERR_INVALID_ARGUMENT;
 * a scalar / STRING / BINARY / DECIMAL end node (use fury_row_project), a non-STRUCT node inside the
 * path or a collection schema as `schema` returns FURY_ERR_UNSUPPORTED.
 *
 * fury_schema_child: the schema of the node the path reaches -- STRUCT: a row schema of its fields
 * (info and hash equal fury_schema_create of those fields); LIST / MAP: the collection schema of that
 * field (as fury_collection_schema_create).  The caller destroys it.  Host only.
 *
 * fury_row_extract, per row r with total = row_offsets[nrows] and B_0 = row_offsets[r]; level k is a
 * struct of n_k fields with a bitmap of bm_k = ((n_k + 63) / 64) * 8 bytes:
 *   1. the header [B_k, B_k + bm_k + 8 n_k) must lie in [0, total) and B_0 must be a multiple of 8
 *      (as take requires of a row), else the value fails;
 *   2. bit path[k] of the bitmap at B_k set: the value is null -- no error, nothing further is read;
 *   3. slot = the int64 at B_k + bm_k + 8 path[k], off = (int32)(slot >> 32), size = (int32)slot as
 *      UnsafeTrait reads them; the value spans [B_k + off, B_k + off + size) and B_{k+1} = B_k + off;
 *   4. the value fails unless off >= 0, size >= 0, both are multiples of 8 (rows, arrays and maps are
 *      8-byte padded by every writer), the span lies in [0, total), an intermediate struct has size >=
 *      bm_{k+1} + 8 n_{k+1}, a final STRUCT has size >= the child's fixed_size (== fixed_size when the
 *      child is_fixed, so that the packed output can be indexed as j * fixed_size) and a final LIST /
 *      MAP has size >= 8.
 * A value that fails is treated as null and FURY_ERR_OUT_OF_BOUNDS is reported on `stream`
 * (fury_device_status), naming source row r -- fury_row_project's "decodes as null and is reported".
 * Nothing outside [rows, rows + total) is read; validating the extracted bytes any deeper belongs to
 * whatever decodes them.
 * Outputs are compact, in row order, shaped like fury_row_filter's: *out_count (device int64,
 * required, never read by the host) = the number of non-null values; out_offsets (required, nrows + 1
 * entries): entries [0, count] are the exclusive scan of the sizes, entries (count, nrows] repeat
 * out_offsets[count]; out_indices (optional, nrows entries): the source row of each entry, -1 past the
 * count; out_validity (optional): an Arrow bitmap, LSB-first, bit r = 1: row r produced an entry,
 * WRITTEN as whole 32-bit words -- 4-byte aligned, (nrows + 31) / 32 words, bits at or past nrows 0;
 * out_rows: the values back to back, capacity and the measure form (out_rows == NULL) exactly as
 * fury_row_take, 8-byte aligned, not overlapping `rows`.  row_offsets is required (a schema with a
 * nested field is never is_fixed).  nrows == 0 writes *out_count = 0 and out_offsets[0] = 0.
 * Asynchronous on `stream`, no host synchronisation; argument errors are returned before any device
 * work, a pending device error of the stream first, as in the other entry points. */
int fury_schema_child(const fury_schema* schema, const int32_t* path, int32_t path_len,
                      fury_schema** out);
int fury_row_extract(const fury_schema* schema, const int32_t* path, int32_t path_len,
                     const void* rows, const int64_t* row_offsets, int64_t nrows,
                     void* out_rows, int64_t out_capacity, int64_t* out_offsets,
                     int64_t* out_count, int64_t* out_indices, uint8_t* out_validity,
                     void* stream);

/* List and map elements as batches -- BinaryArray.getStruct / getArray / getMap (ordinal)
 * (FMT/row/binary/BinaryArray.java:137-150, through UnsafeTrait.java:160-197) and BinaryMap.keyArray()
 * / valueArray() (FMT/row/binary/BinaryMap.java:62-77,101-108) over a batch.  An element slot is
 * (offset << 32) | size relative to the ARRAY's base, and a nested row, array or map addresses its
 * variable-length section relative to its own base, so the bytes an element slot points at are,
 * unchanged, a complete row of the element struct's schema / a complete BinaryArray / BinaryMap.
 * fury_row_explode packs the non-null elements of every row's array into a new batch, which every
 * other entry point takes with the schema fury_schema_element returns: orders[*].price is explode
 * {orders} followed by fury_row_project of price.
 *
 * Which array (both functions, same rules, each message prefixed with the function's name):
 *   - `schema` is a row schema: `path` follows fury_row_extract's rules and must end at a LIST or MAP
 *     (a path ending at a STRUCT returns FURY_ERR_UNSUPPORTED: use fury_row_extract); or
 *   - `schema` is a collection schema: path_len must be 0 (else FURY_ERR_INVALID_ARGUMENT), path may be
 *     NULL, and every batch entry is the array / map itself -- what fury_row_extract or fury_row_encode
 *     of a collection schema produced;
 *   - side 0: the LIST's elements or the MAP's key array; side 1: the MAP's value array.  side 1 on a
 *     LIST, or any other value, returns FURY_ERR_INVALID_ARGUMENT;
 *   - the element type of the chosen array must be STRUCT, LIST or MAP; any other returns
 *     FURY_ERR_UNSUPPORTED (such elements already decode as a flat child column through
 *     fury_decode_prepare / fury_row_project).
 *
 * fury_schema_element: the schema of the output batch -- STRUCT element: a row schema of its fields
 * (info and hash equal fury_schema_create of those fields); LIST / MAP element: the collection schema
 * of the element field (as fury_collection_schema_create).  The caller destroys it.  Host only.
 *
 * fury_row_explode, per row r with total = row_offsets[nrows]:
 *   1. the path is walked exactly as fury_row_extract's steps 1-4 walk it, giving the value's span
 *      [V, V + size), size >= 8, or null, or a failure.  With a collection schema the span is the entry
 *      [row_offsets[r], row_offsets[r + 1]): 8-byte aligned, size >= 8 and a multiple of 8, inside
 *      [0, total), else the row fails;
 *   2. MAP: kb = (int32) of the 8 bytes at V (BinaryMap.pointTo); the row fails unless kb >= 0,
 *      kb % 8 == 0 and 8 + kb <= size.  The key array is [V + 8, V + 8 + kb), the value array
 *      [V + 8 + kb, V + size); the chosen array [A, A + asz) needs asz >= 8.  The other side is never
 *      read (key and value counts that differ are the full decode's error).  LIST: A = V, asz = size;
 *   3. n = (int32) of the int64 at A (BinaryArray.pointTo); the row fails unless n >= 0 and
 *      8 + ((n + 63) / 64) * 8 + 8 n <= asz, so that header and slots lie inside the array;
 *   4. a row that is null or fails has 0 elements; a failure reports FURY_ERR_OUT_OF_BOUNDS on `stream`
 *      (fury_device_status) naming row r;
 *   5. out_list_offsets[0 .. nrows] (device, required) = the exclusive scan of n: the Arrow list
 *      offsets of the column; E = out_list_offsets[nrows];
 *   6. out_entry_validity (optional): bit r = 1: row r has a well-formed, non-null array; written as
 *      whole 32-bit words like fury_row_extract's out_validity.
 * Per element e = out_list_offsets[r] + i, i < n, e < elem_capacity: it is null (no entry, no error)
 * when bit i of the bitmap at A + 8 is set; else off = (int32)(slot >> 32), size = (int32)slot of the
 * slot at A + 8 + ((n + 63) / 64) * 8 + 8 i, and the element fails unless both are >= 0 and multiples
 * of 8, [A + off, A + off + size) lies in [0, total), a STRUCT element has size >= the element
 * schema's fixed_size (== fixed_size when it is_fixed) and a LIST / MAP element has size >= 8.  An
 * element that fails is treated as null and FURY_ERR_OUT_OF_BOUNDS names row r.
 * Outputs are shaped like fury_row_extract's, indexed by element instead of by row: *out_count = the
 * entries produced; out_offsets: elem_capacity + 1 entries, [0, count] the exclusive scan of the
 * sizes, (count, elem_capacity] repeating out_offsets[count]; out_parents (optional, elem_capacity
 * int64): the source row of each entry, -1 past the count; out_ordinals (optional, elem_capacity
 * int32): the entry's ordinal in its array, -1 past the count; out_validity (optional,
 * (elem_capacity + 31) / 32 whole 32-bit words): bit e = 1: element e produced an entry, bits at or
 * past min(E, elem_capacity) 0 -- the Arrow validity of the LIST's child; out_rows / out_capacity: the
 * element values back to back, capacity and the measure form (out_rows == NULL) exactly as
 * fury_row_take.
 * Element capacity: elements at or past elem_capacity are neither produced nor counted, while
 * out_list_offsets is always complete: a caller that sees out_list_offsets[nrows] > elem_capacity
 * grows its buffers and calls again (the fury_row_encode_measured contract).  Every counted element
 * owns an 8-byte slot inside its row's array, so E <= row_offsets[nrows] / 8 for every batch whose
 * rows do not share bytes (every writer's output): elem_capacity = rows bytes / 8 is a bound the host
 * knows without synchronising.  (Malformed slots may point two rows at the same array; E is then still
 * exact and the capacity rule still holds.)
 * The count form, out_offsets == NULL, writes only out_list_offsets and out_entry_validity: out_rows,
 * out_count, out_parents, out_ordinals and out_validity must be NULL, elem_capacity is ignored.
 * Otherwise as fury_row_extract: asynchronous on `stream` with no host synchronisation; a pending
 * device error of the stream is returned first; argument errors (null / misaligned pointers,
 * negative nrows, out_capacity or elem_capacity) are returned before any device work; nrows == 0
 * writes out_list_offsets[0] = 0, *out_count = 0 and out_offsets[0] = 0; `rows` and `out_rows` must
 * not overlap; nothing outside [rows, rows + total) is read and nothing outside the given output
 * extents is written. */
int fury_schema_element(const fury_schema* schema, const int32_t* path, int32_t path_len,
                        int32_t side, fury_schema** out);
int fury_row_explode(const fury_schema* schema, const int32_t* path, int32_t path_len, int32_t side,
                     const void* rows, const int64_t* row_offsets, int64_t nrows,
                     int64_t* out_list_offsets, uint8_t* out_entry_validity,
                     int64_t elem_capacity,
                     void* out_rows, int64_t out_capacity, int64_t* out_offsets, int64_t* out_count,
                     int64_t* out_parents, int32_t* out_ordinals, uint8_t* out_validity,
                     void* stream);

/* A subset of the fields, as rows -- the relational partner of take / filter (Spark's
 * UnsafeProjection): keep, drop and reorder top-level fields without leaving row bytes.  Per row it is
 * BinaryRow's getters feeding a fresh BinaryRowWriter of the selected schema: write(ordinal,
 * <primitive>) for a fixed-width field (FMT/row/binary/writer/BinaryRowWriter.java:86-129),
 * writeUnaligned / write(ordinal, BinaryRow | BinaryArray | BinaryMap) -> writeAlignedBytes / copyTo for
 * a variable-length one (FMT/row/binary/writer/BinaryWriter.java:161-212,243-245).  A variable-length
 * value addresses everything below it relative to its own base, so moving it is a copy of its bytes
 * and one rewritten slot; every field type is allowed, nested ones included.
 *
 * Selection (both functions, same rules, each message prefixed with the function's name):
 * fields[0 .. num_selected) are top-level slots of `schema` in any order, without duplicates,
 * 1 <= num_selected <= num_fields -- there is no cap on the count.  A null table, a count out of
 * range, an index out of range or a duplicate returns FURY_ERR_INVALID_ARGUMENT; a collection schema
 * returns FURY_ERR_UNSUPPORTED.
 *
 * fury_schema_select: the row schema of the selected fields in selection order (names, types,
 * nullability and children kept; info, hash and node count equal fury_schema_create of those fields).
 * The caller destroys it.  Host only.
 *
 * fury_row_select: output row r holds source field fields[j] of source row r in slot j; row count and
 * order are unchanged.  With n, bm, F the source's field count, bitmap bytes and fixed_size, n', bm', F'
 * those of the selected schema, total = row_offsets[nrows] and B = row_offsets[r] (r * F when the source
 * is_fixed: a non-NULL row_offsets is then ignored, as in fury_row_project), per row:
 *   1. B must be a multiple of 8, [B, B + F) must lie in [0, total) and the row's own extent
 *      (row_offsets[r + 1] - B) must be >= F (fury_row_update's rule); otherwise the ROW fails: its
 *      output is F' bytes with bitmap bits [0, n') set and every slot 0, and FURY_ERR_OUT_OF_BOUNDS is
 *      reported on `stream` (fury_device_status) naming row r;
 *   2. source bit k = fields[j] set: output bit j is set and slot j is 0; the source slot is not read;
 *   3. a fixed-width field of width w: slot j = bytes [0, w) of the source slot, zero-extended to 8
 *      bytes; a BOOL byte becomes 1 when non-zero, else 0;
 *   4. a variable-length field: off = (int32)(slot >> 32), size = (int32)slot.  The VALUE fails unless
 *      off >= 0, size >= 0, off % 8 == 0 (every writer places values at the 8-aligned writer index),
 *      [B + off, B + off + size) lies in [0, total), a DECIMAL has size == 16, a STRUCT / LIST / MAP has
 *      size % 8 == 0 with size >= the child's header (bitmap + 8 per field) for a STRUCT and size >= 8 for
 *      a LIST / MAP.  A failed value becomes null as in 2 and FURY_ERR_OUT_OF_BOUNDS names row r.  A
 *      valid one is copied unchanged to the row's current end W (W starts at F' and advances in
 *      selection order), the tail up to the next multiple of 8 is zeros (source padding is not copied),
 *      slot j = (W << 32) | size, and W advances by size rounded up to 8; a size-0 value still gets its
 *      slot.  Should W exceed INT32_MAX - 7 the row fails as in 1 (only rows whose slots alias one
 *      large span get there);
 *   5. the row's size is the final W, a multiple of 8.
 * out_offsets[0 .. nrows] is the exclusive scan of the row sizes.  out_rows, out_capacity and the
 * measure form (out_rows == NULL) behave exactly as in fury_row_take: bytes at or past the capacity are
 * never written, out_offsets is always complete.  When the selected schema is_fixed, output row r sits
 * at r * F', out_offsets may be NULL, and out_rows != NULL with out_capacity < nrows * F' returns
 * FURY_ERR_CAPACITY before any device work; otherwise out_offsets is required.  row_offsets is required
 * unless the source is_fixed.  nrows == 0 writes out_offsets[0] = 0 when given.
 * For rows any writer made the result equals fury_row_encode of the selected columns under the selected
 * schema byte for byte, and selecting every field in order returns the source bytes; for any input the
 * output is canonical (zero padding, zero null slots, zero upper slot bytes).
 * `rows` and `out_rows` are 8-byte aligned and must not overlap; nothing outside [rows, rows + total)
 * is read and nothing outside [out_rows, out_rows + min(out_capacity, needed)) and out_offsets is
 * written.  Asynchronous on `stream`, no host synchronisation; argument errors are returned before any
 * device work, a pending device error of the stream first. */
int fury_schema_select(const fury_schema* schema, const int32_t* fields, int32_t num_selected,
                       fury_schema** out);
int fury_row_select(const fury_schema* schema, const int32_t* fields, int32_t num_selected,
                    const void* rows, const int64_t* row_offsets, int64_t nrows,
                    void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* The fields of several row batches joined row by row -- fury_row_select generalised from one source
 * to several: add a computed column to existing rows, replace a field of any type, re-join two halves
 * that were processed separately.  Per row it is the getters of several BinaryRows feeding one fresh
 * BinaryRowWriter of the combined schema, with the writer calls fury_row_select names; a
 * variable-length value addresses everything below it relative to its own base, so it moves into
 * another row as its bytes and one rewritten slot, whichever row it came from.
 *
 * Picks (both functions, same rules, each message prefixed with the function's name): 1 <= num_sources
 * <= FURY_ZIP_MAX_SOURCES row schemas; picks holds 2 * num_picks int32 words, pick j = (source index,
 * top-level slot of that source), num_picks >= 1 with no upper limit, in any order, the same (source,
 * slot) pair at most once.  A source that no pick names is allowed and is never read (its rows and
 * row_offsets may be NULL).  A null table, a count out of range, a source index outside [0,
 * num_sources), a slot outside its source or a duplicate pair returns FURY_ERR_INVALID_ARGUMENT; a
 * collection schema among the sources returns FURY_ERR_UNSUPPORTED.
 *
 * fury_schema_zip: the row schema of the picked fields in pick order (names, types, nullability and
 * children kept; info, hash and node count equal fury_schema_create of those fields; equal names from
 * different sources are kept as they are).  The caller destroys it.  Host only.
 *
 * fury_row_zip: output row r holds, in slot j, field picks[j] of row r of its source; every source has
 * nrows rows.  With B, F, bm and total those of the pick's source s (row_offsets NULL or ignored when
 * that source is_fixed: row r at r * F_s) and n', bm', F' those of the zipped schema, each picked field
 * follows rules 2-4 of fury_row_select unchanged.  Rule 1 holds per source: if row r of source s
 * starts off an 8-byte boundary, its header leaves [0, total_s) or its own extent is shorter than F_s,
 * every field picked from s is null in output row r (bit set, slot 0, no payload), the fields of the
 * other sources are unaffected, and FURY_ERR_OUT_OF_BOUNDS names row r.  W starts at F' and advances in
 * pick order across all sources; should it exceed INT32_MAX - 7 the whole output row is all null, as
 * in fury_row_select.  out_offsets, out_rows, out_capacity, the measure form (out_rows == NULL), the
 * fixed form (a zipped schema that is_fixed: row r at r * F', out_offsets may be NULL, FURY_ERR_CAPACITY
 * before any device work when the buffer is too small; otherwise out_offsets is required) and nrows ==
 * 0 are those of fury_row_select; the output is canonical for any input.
 * Consequences: with one source, the output and the reported rows equal fury_row_select of the same
 * slots, for any input bytes; for rows any writer made, the output equals fury_row_encode of the picked
 * columns under the zipped schema byte for byte; zipping fury_row_select(A, S1) and fury_row_select(A,
 * S2) with the picks that restore A's field order returns A's bytes.
 * Every rows and out_rows is 8-byte aligned; out_rows must not overlap any source, sources may alias
 * each other.  Nothing outside [rows_s, rows_s + total_s) of a source is read and nothing outside
 * [out_rows, out_rows + min(out_capacity, needed)) and out_offsets is written.  Asynchronous on
 * `stream`, no host synchronisation; argument errors are returned before any device work, a pending
 * device error of the stream first. */
#define FURY_ZIP_MAX_SOURCES 4
typedef struct fury_zip_source {
  const fury_schema* schema;     /* a row schema (not a collection schema) */
  const void* rows;              /* device, 8-byte aligned */
  const int64_t* row_offsets;    /* nrows + 1 entries; ignored (may be NULL) when schema is_fixed */
} fury_zip_source;
int fury_schema_zip(const fury_schema* const* schemas, int32_t num_sources,
                    const int32_t* picks, int32_t num_picks, fury_schema** out);
int fury_row_zip(const fury_zip_source* sources, int32_t num_sources,
                 const int32_t* picks, int32_t num_picks, int64_t nrows,
                 void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* Elements and nested values back into rows -- the inverses of fury_row_explode and fury_row_extract.
 * A nested row, array or map addresses everything below it relative to its own base, so re-nesting a
 * value is a copy of its bytes plus a small generated header: per row the batch form of
 * BinaryArrayWriter.reset(n) followed by write(ordinal, BinaryRow | BinaryArray | BinaryMap) or
 * setNullAt(ordinal) (FMT/row/binary/writer/BinaryArrayWriter.java:91-129,
 * FMT/row/binary/writer/BinaryWriter.java:106-114,243-245; cpp/fury/row/writer.cc), and of a one-field
 * BinaryRowWriter.write(0, BinaryRow | BinaryArray | BinaryMap).  With fury_row_zip the loop closes on
 * the device, as bytes: explode -> process the elements -> implode -> zip back into the parent rows.
 *
 * Target (`schema` is the TARGET's schema; each message is prefixed with the function's name):
 *   - fury_row_implode, rows form: a row schema with exactly one field, a LIST of STRUCT / LIST / MAP;
 *     output row r is [8-byte bitmap][slot][array];
 *   - fury_row_implode, collection form: a LIST collection schema (fury_collection_schema_create) with
 *     such an element; output entry r is the array itself and entry_validity must be NULL
 *     (FURY_ERR_INVALID_ARGUMENT);
 *   - fury_row_wrap: a row schema with exactly one field, a STRUCT, LIST or MAP;
 *   - FURY_ERR_UNSUPPORTED: a row schema with more than one field (join further fields with
 *     fury_row_zip); a scalar / STRING / BINARY / DECIMAL element or value; a MAP as implode's target
 *     (assembling a map needs a scalar key array, which fury_row_explode does not produce: build the
 *     value array with implode's collection form and put it next to a key array with
 *     fury_row_map_join); a collection schema as wrap's target.
 *
 * Inputs of both: values / value_offsets (num_values + 1 device int64) are a compact batch of values in
 * order -- exactly what fury_row_explode and fury_row_extract write to out_rows / out_offsets;
 * VT = value_offsets[num_values] is the buffer's length.  num_values = explode's elem_capacity is
 * valid: the entries past the count repeat the total and are never referenced.  value_offsets is always
 * required.  Validity bitmaps are Arrow bitmaps, LSB-first, 1 = present, READ as whole 32-bit words
 * (4-byte aligned, readable to a multiple of 4 bytes; bits at or past the count are ignored), NULL =
 * all present.  A present element (implode) or row (wrap) takes the next value in order: its value
 * index v is the rank of its bit, the number of 1 bits before it in the whole bitmap.
 *
 * Value check: value v is well-formed when v < num_values, 0 <= value_offsets[v] <= value_offsets[v + 1]
 * <= VT, start and size are multiples of 8 and size >= least -- a STRUCT's fixed_size (bitmap + 8 per
 * field), 8 for a LIST or MAP.  A value that fails makes its element (implode) or row (wrap) null,
 * none of its bytes are copied, and FURY_ERR_OUT_OF_BOUNDS is reported on `stream`
 * (fury_device_status) naming the output row.
 *
 * fury_row_implode, per row r with n = list_offsets[r + 1] - list_offsets[r] (list_offsets: nrows + 1
 * device int64, the Arrow list offsets fury_row_explode wrote; elements are numbered [0, num_elements)):
 *   1. the row fails unless 0 <= list_offsets[r] <= list_offsets[r + 1] <= num_elements and
 *      n <= (INT32_MAX - 15) / 8 (BinaryArrayWriter's MAX_ROUNDED_ARRAY_LENGTH rule);
 *   2. array bytes, bm = ((n + 63) / 64) * 8: int64 n; bm bitmap bytes, bit i = 1 when element i is
 *      null (its elem_validity bit is 0 or its value failed), bits at or past n 0; n slots, 0 for a null
 *      element, else (off << 32) | size with off relative to the array's base; then the present
 *      elements' bytes back to back in ordinal order from 8 + bm + 8 n;
 *   3. the array's size A = 8 + bm + 8 n + the kept value bytes; the row fails if 16 + A (rows form) or
 *      A (collection form) exceeds INT32_MAX - 7;
 *   4. rows form, row present: bitmap word 0, slot (16 << 32) | A, array; the row's size is 16 + A;
 *   5. rows form, row null (entry_validity bit 0) or failed: 16 bytes, bit 0 set, slot 0.  A failed
 *      row is reported; a null row is not, whatever its list_offsets range holds and whichever values
 *      its elements would have taken;
 *   6. collection form, row failed: an empty array (8 bytes, n = 0), reported;
 *   7. ranks always count over the whole elem_validity, also through null and failed rows, and a value
 *      no present row's range covers is never reported.
 *
 * fury_row_wrap, per row r: a present row (validity bit 1) whose value passes the value check and has
 * 16 + size <= INT32_MAX - 7 gives [bitmap word 0][(16 << 32) | size][the value's bytes]; a null or
 * failed row gives 16 bytes with bit 0 set and slot 0 (failed: reported).
 *
 * Both: out_offsets[0 .. nrows] (required) is the exclusive scan of the sizes; out_rows, out_capacity
 * and the measure form (out_rows == NULL) behave exactly as in fury_row_take: bytes at or past the
 * capacity are never written, out_offsets is always complete.  nrows == 0 writes out_offsets[0] = 0.
 * Asynchronous on `stream`, no host synchronisation; a pending device error of the stream is returned
 * first; argument errors (null or misaligned pointers, negative counts or capacity) are returned
 * before any device work; nrows or num_elements of 2^38 or more is FURY_ERR_INVALID_ARGUMENT.
 * `values` and `out_rows` are 8-byte aligned and must not overlap.  Nothing outside [values, values +
 * VT), the given bitmaps and the given offsets arrays is read; nothing outside [out_rows, out_rows +
 * min(out_capacity, needed)) and out_offsets is written.
 * Consequences, for rows any writer made: implode(explode(X, {f})) in rows form equals
 * fury_row_select(X, {f}) byte for byte; in collection form it equals fury_row_extract(X, {f}) when no
 * row is null; wrap(extract(X, {f})) equals fury_row_select(X, {f}); each equals fury_row_encode of the
 * same columns under the target schema.  For any input the output is canonical: zero null slots, zero
 * bitmap bits at or past n. */
int fury_row_implode(const fury_schema* schema,
                     const void* values, const int64_t* value_offsets, int64_t num_values,
                     const int64_t* list_offsets, int64_t nrows,
                     const uint8_t* entry_validity, const uint8_t* elem_validity,
                     int64_t num_elements,
                     void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);
int fury_row_wrap(const fury_schema* schema,
                  const void* values, const int64_t* value_offsets, int64_t num_values,
                  const uint8_t* validity, int64_t nrows,
                  void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* Maps as key / value arrays and back -- BinaryMap.keyArray() / valueArray()
 * (FMT/row/binary/BinaryMap.java:62-77,101-108) and the constructor BinaryMap(BinaryArray keys,
 * BinaryArray values, Field) (BinaryMap.java:52-60; the writer side is serializeForMap:
 * writeDirectly(-1), the key array, writeDirectly(offset, keyArraySize), the value array) over a batch.
 * A map is [int64 keyArrayBytes][key BinaryArray][value BinaryArray] and each array addresses its
 * contents relative to its own base, so both directions are byte copies plus one generated 8-byte
 * word.  An array batch is a batch under a LIST collection schema: fury_row_encode /
 * fury_decode_prepare encode and decode it (scalar, STRING or DECIMAL keys), fury_row_explode /
 * fury_row_implode in collection form take it (STRUCT / LIST / MAP values).  With them every map shape
 * is processable on the device: split -> (decode + re-encode the key array, or explode -> process ->
 * implode the value array) -> join -> fury_row_zip.
 *
 * Which map (fury_schema_map_side and fury_row_map_split, same rules, each message prefixed with the
 * function's name): `schema` is a row schema and `path` follows fury_row_extract's rules and must end at
 * a MAP, or `schema` is a MAP collection schema and path_len is 0 (else FURY_ERR_INVALID_ARGUMENT; path
 * may be NULL).  A path that ends at a STRUCT or LIST, or a LIST collection schema, returns
 * FURY_ERR_UNSUPPORTED.
 *
 * fury_schema_map_side: the LIST collection schema of the key array (side 0) or the value array (side
 * 1; any other value returns FURY_ERR_INVALID_ARGUMENT) -- info, node count and hash (0) equal
 * fury_collection_schema_create of a LIST field (the map's name and nullability) whose element is the
 * map's key / value field.  The caller destroys it.  Host only.
 *
 * fury_row_map_split, per row r with total = row_offsets[nrows]:
 *   1. the path is walked exactly as fury_row_explode's steps 1-2 walk it, collection form included,
 *      giving the map's span [V, V + size), size >= 8, or null, or a failure;
 *   2. kb = (int32) of the 8 bytes at V (BinaryMap.pointTo); the row fails unless kb >= 0, kb % 8 == 0
 *      and 8 + kb <= size;
 *   3. the key array is K = [V + 8, V + 8 + kb), the value array A = [V + 8 + kb, V + size); the row
 *      fails unless both are >= 8 bytes;
 *   4. n_k, n_v = (int32) of the int64 at the start of each array; the row fails unless
 *      n_k == n_v >= 0 (BinaryMap.pointTo:73-75);
 *   5. per side the row fails unless 8 + ((n + 63) / 64) * 8 + round_up_8(n * w) <= that array's size,
 *      w the element's slot width (fury_type_width; 8 for a variable-length or nested element);
 *   6. nothing below the two array headers is read or checked: the arrays move as bytes, and
 *      validating them any deeper belongs to whatever decodes them;
 *   7. a null row has no entry and no error;
 *   8. a failed row has no entry and FURY_ERR_OUT_OF_BOUNDS is reported on `stream`
 *      (fury_device_status) naming row r; a failure of n_k == n_v reports the same status and its
 *      message says that the element counts differ.
 * Outputs are shaped like fury_row_extract's, one batch per side: *out_count, out_indices and
 * out_validity (whole 32-bit words) are shared -- entry validity is decided on both headers, so the two
 * batches always have the same entries --; per side nrows + 1 offsets (entries [0, count] the exclusive
 * scan of the array sizes, entries (count, nrows] repeating the total), the arrays back to back, its own
 * capacity and its own measure form (out_keys / out_values NULL with its offsets given), all exactly
 * as fury_row_extract's out_rows / out_capacity / out_offsets.  A side whose offsets pointer is NULL is
 * skipped (its buffer must be NULL too) and never read beyond its header; both sides NULL returns
 * FURY_ERR_INVALID_ARGUMENT.  nrows == 0 writes *out_count = 0 and [0] = 0 of each given offsets array.
 *
 * fury_row_map_join: `schema` is the TARGET's schema, in the two forms of fury_row_implode --
 *   - rows form: a row schema with exactly one field, a MAP; output row r is [bitmap word
 *     0][(16 << 32) | M][map];
 *   - collection form: a MAP collection schema; output entry r is the map itself and validity must be
 *     NULL (FURY_ERR_INVALID_ARGUMENT);
 *   - FURY_ERR_UNSUPPORTED: a row schema with more than one field (join further fields with
 *     fury_row_zip); a field or collection that is not a MAP.
 * keys / key_offsets and values / value_offsets are two compact batches of num_values entries each --
 * exactly what fury_row_map_split writes; KT = key_offsets[num_values] and VT =
 * value_offsets[num_values] are the buffers' lengths.  validity is one Arrow bitmap read as
 * fury_row_wrap reads it (whole 32-bit words, NULL = all present).  Per row r:
 *   1. a present row takes entry v of BOTH batches, v the rank of its bit;
 *   2. each of the two entries must pass fury_row_implode's value check with least = 8, against its own
 *      buffer's length: v < num_values, 0 <= start <= end <= KT (VT), start and size multiples of 8,
 *      size >= 8;
 *   3. n_k, n_v = the int64 at each entry's start must be equal and in [0, (INT32_MAX - 15) / 8]
 *      (BinaryArrayWriter's MAX_ROUNDED_ARRAY_LENGTH); nothing else of an entry is checked;
 *   4. with ksz, vsz the entries' sizes, M = 8 + ksz + vsz; the row fails if 16 + M (rows form) or M
 *      (collection form) exceeds INT32_MAX - 7;
 *   5. a present, well-formed row writes the map: int64 ksz, the key entry's bytes, the value entry's
 *      bytes;
 *   6. rows form, row null (validity bit 0) or failed: 16 bytes, bit 0 set, slot 0.  A failed row is
 *      reported (FURY_ERR_OUT_OF_BOUNDS naming row r, saying so when the counts differ); a null row is
 *      not;
 *   7. collection form, row failed: the empty map, 24 bytes (int64 8, int64 0, int64 0), reported.
 * out_offsets, out_rows, out_capacity, the measure form, nrows == 0, the argument errors, the
 * asynchrony and the read / write extents are fury_row_wrap's, with [keys, keys + KT) and [values,
 * values + VT) for its one input buffer; neither input buffer may overlap out_rows (they may alias
 * each other).
 *
 * Consequences, for rows any writer made: join(split(X, {m})) in rows form equals fury_row_select(X,
 * {m}) byte for byte; in collection form it equals fury_row_extract(X, {m}) when no row is null; each
 * side of split(X) equals fury_row_encode, under that side's collection schema, of the map column's key
 * / value child with the map's offsets; fury_row_explode(X, path, side) equals fury_row_explode in
 * collection form (side 0) of split's batch for that side.
 * Both: asynchronous on `stream`, no host synchronisation; a pending device error of the stream is
 * returned first; argument errors (null or misaligned pointers, negative counts or capacities) are
 * returned before any device work; nrows of 2^38 or more is FURY_ERR_INVALID_ARGUMENT.  Every buffer is
 * 8-byte aligned and no output overlaps an input; split reads nothing outside [rows, rows + total),
 * and neither writes outside [out, out + min(capacity, needed)) of a buffer and the given arrays. */
int fury_schema_map_side(const fury_schema* schema, const int32_t* path, int32_t path_len,
                         int32_t side, fury_schema** out);
int fury_row_map_split(const fury_schema* schema, const int32_t* path, int32_t path_len,
                       const void* rows, const int64_t* row_offsets, int64_t nrows,
                       void* out_keys, int64_t key_capacity, int64_t* out_key_offsets,
                       void* out_values, int64_t value_capacity, int64_t* out_value_offsets,
                       int64_t* out_count, int64_t* out_indices, uint8_t* out_validity,
                       void* stream);
int fury_row_map_join(const fury_schema* schema,
                      const void* keys, const int64_t* key_offsets,
                      const void* values, const int64_t* value_offsets, int64_t num_values,
                      const uint8_t* validity, int64_t nrows,
                      void* out_rows, int64_t out_capacity, int64_t* out_offsets, void* stream);

/* Appends the Arrow columns `src` (src_rows top-level entries, e.g. fury_rows_to_arrow /
 * fury_decode_execute output) at entry dst_rows of the columns `dst` -- ArrowWriter.write(row)
 * appending at rowCount until finish() / reset() (FMT/vectorized/ArrowWriter.java:74-99): values
 * and STRING/BINARY payloads are copied after the destination's, offsets rebased on its end
 * (offsets[dst_rows]), validity / BOOL bits shifted to its bit position, LIST / MAP child entries
 * appended after its child entries, STRUCT children entry-aligned.  Every node's destination
 * buffers must hold the combined entries (validity / BOOL bitmaps as 32-bit words: 4-byte aligned,
 * padded to a multiple of 4 bytes; offsets entries + 1); fury_column.capacity, when > 0, bounds a
 * node's values / payload bytes (FURY_ERR_CAPACITY).  Child offsets of `src` must start at 0.
 * Reads the destination's and source's end offsets from the device, so the call synchronises
 * `stream`; the copies themselves are one launch on it. */
int fury_arrow_append(const fury_schema* schema, fury_column* dst, int64_t dst_rows,
                      const fury_column* src, int64_t src_rows, void* stream);

/* ---- ArrayEncoder / MapEncoder batches (Encoders.arrayEncoder / mapEncoder,
 *      FMT/encoder/Encoders.java:230-600, ArrayEncoderBuilder.java:118-140,
 *      MapEncoderBuilder.java:152-208) ----------------------------------------------------- */
/* A collection schema: its batch entries are top-level BinaryArrays (`field` of type LIST:
 * ArrayEncoder.toArray(obj)) or BinaryMaps (`field` of type MAP: [int64 keyArrayBytes][key
 * BinaryArray][value BinaryArray], MapEncoder.toMap(obj)) instead of rows.  The batch entry points
 * take it unchanged: fury_row_measure / fury_row_encode / fury_row_encode_measured write entry i
 * at row_offsets[i] (every entry a multiple of 8 bytes), fury_decode_prepare /
 * fury_decode_execute decode.  `columns` is ONE column, the collection column itself (LIST:
 * offsets + element child; MAP: offsets + child [keys, values]) with validity NULL: a collection
 * handed to toArray / toMap is never null.  schema_hash is 0 (these encoders carry no hash; their
 * encode(MemoryBuffer, T) frames [int32 size][bytes]), and the row framing entry points return
 * FURY_ERR_UNSUPPORTED for them. */
int fury_collection_schema_create(const fury_field* field, fury_schema** out);

/* ---- nested schemas: two-step decode --------------------------------------------------- */
/* Schemas with STRUCT / MAP / LIST-of-variable-length fields produce a TREE of Arrow columns whose
 * sizes depend on the data.  Nodes are the schema's fields at every level, numbered breadth-first:
 * top-level fields 0..n-1 first, then each node's children contiguously (LIST: element; STRUCT:
 * its fields; MAP: key, value).  fury_decode_prepare counts, for every node, the Arrow entries
 * (node_entries) and STRING/BINARY payload bytes (node_bytes) the batch produces and returns a
 * plan; the caller allocates every node's buffers (validity and BOOL value bitmaps ZEROED, offsets
 * entries+1, values entries*width / node_bytes / 16*entries) and runs fury_decode_execute on
 * the column tree (fury_column.child: LIST -> element column; STRUCT -> its field columns; MAP ->
 * [keys, values]).  Flat schemas may use it too.  Synchronises `stream` once (prepare). */
typedef struct fury_decode_plan fury_decode_plan;
int32_t fury_schema_num_nodes(const fury_schema* schema);
int fury_decode_prepare(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                        int64_t nrows, int64_t* node_entries, int64_t* node_bytes,
                        fury_decode_plan** plan, void* stream);
int fury_decode_execute(fury_decode_plan* plan, fury_column* columns, int32_t arrow, void* stream);
void fury_decode_plan_destroy(fury_decode_plan* plan);

/* ---- asynchronous device errors (no reference equivalent) ------------------------------- */
/* Decode kernels report what they find ASYNCHRONOUSLY: fury_row_decode,
 * fury_rows_to_arrow and fury_decode_execute return before their kernels run, so a malformed
 * batch is reported later --
 *   FURY_ERR_OUT_OF_BOUNDS  a variable-length value, array or map header outside the batch's row
 *                           bytes (MemoryBuffer's IndexOutOfBoundsException), or a nested row
 *                           whose slots alias other bytes so that its walk would visit more
 *                           items than twice its bytes (found by fury_decode_prepare);
 *   FURY_ERR_UNSUPPORTED    map key / value arrays of different lengths (BinaryMap.pointTo);
 *   FURY_ERR_DEVICE         a decoupled look-back that gave up waiting (by construction -- a
 *                           look-back computes a silent predecessor's aggregate itself -- never
 *                           raised on working hardware).
 * The report goes to the STREAM the call was launched on (the legacy null stream: per host
 * thread): fury_device_status(stream) synchronises that stream and returns it, and the next entry
 * point called on the same stream returns it before doing anything (without synchronising: it sees
 * the kernels that have finished).  Either clears it.  Calls on other streams never see it.  When
 * one is reported, every output of the failing call is invalid (the values that failed decode as
 * null; the rest may be incomplete).  fury_decode_prepare and the host-memory entry points
 * synchronise and report their own batch's errors directly.
 * Each stream that launched work holds one of 1024 error slots until it is released: call
 * fury_stream_release(stream) (it synchronises the stream and drops any unreported error) before
 * destroying a stream passed to this library; streams the library creates itself, and the
 * per-thread keys of the null stream / hipStreamPerThread, are released by the library.  With
 * every slot held, the next call on a new stream fails with FURY_ERR_DEVICE (slots are never
 * shared between streams). */
int fury_device_status(void* stream);
int fury_stream_release(void* stream);

/* ---- workspace (no reference equivalent) ------------------------------------------------- */
/* The library caches the device workspaces of its calls (scan scratch, decode plans, column
 * tables; at most 2 GB of idle blocks per process).  Releases every idle cached block of `device`
 * (after the work that last used it, so the call may wait for it) and trims the device's stream
 * memory pool.  An allocation that fails does the same by itself before it reports. */
int fury_trim_workspace(int32_t device);

/* ---- tuning (no reference equivalent) ---------------------------------------------------- */
/* Process-wide knobs for tests and A/B measurement (results are identical under every value,
 * except the diagnostics "walk_skip" and "var_skip").  fury_set_tuning returns FURY_OK, or
 * FURY_ERR_INVALID_ARGUMENT for an unknown key or a value outside the key's legal values (the
 * knob keeps its value; fury_last_error names the legal ones).  Byte sizes marked (16) are stored,
 * and read back, rounded up to a multiple of 16.  fury_get_tuning returns the value, or -1 for an
 * unknown key.
 * Key "lookback_help" (0 / 1): 1 = every look-back of the variable-length decode computes a silent
 * predecessor tile's aggregate at once (the path a late-dispatched predecessor takes).
 * Key "unframe": 0 speculative parallel stream parse (a stream that does not verify -- a payload
 * spelling a plausible header -- is repaired in parallel; the sequential walk only reports
 * errors), 1 always the sequential walk.
 * Nested engines: "nested_decode" 2 row walk (default), 1 level engine (schemas past the walk's
 * limits -- 5 levels, 256 counted nodes -- use it by themselves), 3 row walk with the tile BFS past
 * its limits, 4 tile BFS ("bfs_threads" 64 / 128 / 256 / 512, default 128; "bfs_rows" 1 .. 4096,
 * default 128; "bfs_stage", "bfs_arena" 0 .. 131072 bytes (16), 0 = sized from the batch;
 * fury_get_tuning "bfs_fallbacks" = batches whose tiles outgrew the arena and went to the walk /
 * level engine); nested encode is the row walk with an explicit-stack continuation for deep
 * schemas: "rowenc_rows" (128 / 256 / 512 threads per group, default 256), "rowenc_tile" (rows per
 * group, 0 .. 256, 0 = threads), "rowenc_img" (LDS image bytes, 1024 .. 155648 (16), default
 * 77824); row-walk decode "walk_threads" (64 / 128 / 256, default 128), "walk_threads_write" (64 /
 * 128 / 256 / 512, default 512), "walk_stage" / "walk_stage_write" / "walk_pool" / "walk_out" (LDS
 * bytes, 0 .. 98304 (16); defaults 12288 / 0 / 8192 / 40960), "walk_prefetch" (0 .. 3: bit 0 write
 * pass, default; bit 1 count pass), "walk_group_k" / "walk_group_min" (0 .. 256: a schema with more
 * than walk_group_min counted nodes, default 16, walks its top-level fields in groups of about
 * walk_group_k counted nodes, default 8, a workgroup per tile and group; 0 = one group); flat
 * schemas of 17-256 fields: "var_wide" (1 wide tiles, default; 0 generic var tiles), "wide_engine"
 * (the plan's engine for them: 0 auto -- the row walk when the batch's average row exceeds
 * "wide_walk_row" bytes, any value >= 0, default 896 --, 1 wide tiles, 2 row walk;
 * "wide_enc_engine" the same for the encode, by the columns' estimated row), "wide_threads" /
 * "wide_enc_threads" (256 / 512 / 1024, defaults 256 / 512); diagnostics "var_skip" (0 .. 255,
 * register-staged encode / decode phases skipped: outputs WRONG, timing only), "tree_debug" (0 / 1,
 * phase clocks; set only, fury_get_tuning returns -1) and "walk_skip" (0 .. 15, bitmask of
 * write-pass phases skipped: outputs WRONG, timing only).  Variable-length decode tile plan:
 * "var_dec_cover" (percent of a tile's row bytes the LDS stage must hold, 50 .. 100, default 95; 0
 * sets the default), "var_dec_rows" (forced tile rows, 64 .. 512 in steps of 64, 0 = plan),
 * "var_dec_pipe" (0 one tile per workgroup, default; 1 / 2 persistent workgroups with two row
 * stages, the 3- and 6-column instances -- measured slower, kept for A/B).  Fixed-width encode:
 * "fixed_enc" (column loads per lane in flight: 2 = 16, default; 0 = 8; 3 = 32; 4 = 16 with 8
 * stores; 1 = 16-B pair loads), "fixed_enc_tail_kib" (KiB of trailing row bytes of a batch that
 * the fast-path encode stores with the default cache policy, the rows in front of them
 * non-temporally: 0 .. 4194304, default 524288 = 512 MiB; 0 = every row non-temporal).
 * Fixed-width decode: "fixed_dec" (0 = 8 column stores per lane in flight, default; 1 = 16; 2 = 4;
 * 3 = 8 with 8 row loads per lane in flight instead of 16).
 * Host path: "host_decode_inplace" (0 / 1).
 * fury_get_tuning only (fury_set_tuning refuses them as unknown keys): "unframe_walks" = streams
 * the walk parsed (wholly or from the first frame the repair could not place), "unframe_repairs" =
 * streams the parallel repair parsed,
 * "host_direct" = fury_row_encode_host / _decode_host calls that ran their kernels directly on
 * pinned host buffers (fixed-width and flat variable-length schemas, no staging),
 * "lookback_timeouts" = decoupled look-backs that gave up (must stay 0; synchronous device read),
 * "err_slots" = device error slots held by live streams (fury_stream_release),
 * "err_slots_quarantined" = slots of exited threads waiting for a device synchronisation,
 * "thread_key_exits" = threads that exited holding per-thread slot keys, "err_slot_last_key" = the
 * key the last slot was assigned under (0 a stream handle, 1 a thread's key) -- diagnostics,
 * "decode_budget_errors" = nested decodes refused by the item budget (a device limit),
 * "var_dec_rows_rejected" = forced "var_dec_rows" tiles whose images did not fit (planned tile used). */
int fury_set_tuning(const char* key, int32_t value);
int32_t fury_get_tuning(const char* key);

/* ---- measurement (no reference equivalent) ------------------------------------------------ */
/* Same-device streaming copy of `bytes` (a positive multiple of 16 KB) from src to dst (device,
 * 16-byte aligned) with 16-B non-temporal loads / stores, asynchronous on `stream`: the box's
 * achievable copy rate, which bench.py reports beside the codec's roofline fraction. */
int fury_hbm_copy(void* dst, const void* src, int64_t bytes, void* stream);

/* ---- framing (Encoders.java:201-213 / 165-182) ------------------------------------------ */
/* Writes the stream RowEncoder.encode(MemoryBuffer, T) produces for each row in turn:
 * [int32 len = 8 + rowSize][int64 schemaHash][row bytes].  frame_offsets (device, nrows+1)
 * receives where each frame starts; frame i starts at row_offsets[i] + 12 * i. */
int fury_frame_rows(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                    int64_t nrows, void* out, int64_t* frame_offsets, void* stream);
/* Parses such a stream back (RowEncoder.decode(MemoryBuffer) nrows times): writes
 * row_offsets[0..nrows] and the rows packed into `rows_out`, checking every schemaHash; a
 * mismatch returns FURY_ERR_CLASS_NOT_COMPATIBLE, a frame past the end FURY_ERR_OUT_OF_BOUNDS.
 * `stream_bytes` may start at any byte address.  Parallel on the device (speculative header scan
 * + verify, parallel repair when a payload spells a header).  Synchronises `stream`. */
int fury_unframe_rows(const fury_schema* schema, const void* stream_bytes, int64_t stream_len,
                      int64_t nrows, void* rows_out, int64_t* row_offsets, void* stream);

/* ---- host-memory batch path (the JNI boundary: DirectByteBuffer addresses) ---------------- */
/* The functions below take HOST pointers (a JVM's off-heap buffers) and run the device path
 * inside the call (synchronous): Encoders.bean(...).encode over a batch
 * (FMT/encoder/Encoders.java:185-213) and decode (:165-182), with the bytes crossing PCIe.
 * Fixed-width schemas whose buffers are ALL pinned (fury_host_alloc or fury_host_register) run
 * the kernel directly on host memory — loads and stores cross PCIe in both directions at once,
 * no HBM staging ("host_direct" counts these calls); otherwise they are staged through HBM
 * (chunked over three HIP streams).  Flat variable-length schemas on pinned buffers run direct
 * too (bitmaps through HBM), and so does the ENCODE of nested schemas (the column tree read and
 * the rows written in place); otherwise they are staged whole.  `device` is the
 * HIP device ordinal.  Buffers from fury_host_alloc (hipHostMalloc) run fastest; registering
 * ordinary 4 KB-page memory (fury_host_register, hipHostRegister) pins it in place but the GPU
 * then walks 4 KB translations (host path). */
int fury_host_alloc(int64_t bytes, void** out);  /* pinned host memory, freed by fury_host_free */
int fury_host_free(void* ptr);
int fury_host_register(void* ptr, int64_t bytes);
int fury_host_unregister(void* ptr);
/* Host columns (fury_column layout, host pointers) -> host rows.  Fixed-width: rows are
 * nrows * fixed_size bytes, row_offsets optional (filled with i * fixed_size when given).
 * Variable-length: row_offsets (host, nrows + 1) is required and filled.  *row_bytes = bytes
 * the rows need; FURY_ERR_CAPACITY (nothing written) when that exceeds rows_capacity. */
int fury_row_encode_host(const fury_schema* schema, const fury_column* columns, int64_t nrows,
                         void* rows, int64_t rows_capacity, int64_t* row_offsets,
                         int64_t* row_bytes, int32_t device);
/* Host rows -> host columns (fromRow semantics, like fury_row_decode).  Variable-length flat
 * schemas: STRING/BINARY payload capacity in fury_column.capacity, LIST element bytes in the
 * child's capacity (FURY_ERR_CAPACITY when short: staged calls size first and write nothing,
 * direct calls write nothing past a capacity and leave offsets[nrows] = the size needed); nested
 * schemas and flat ones with more than 256 fields of which some are variable-length:
 * FURY_ERR_UNSUPPORTED (their output sizes depend on the data: fury_decode_host_prepare /
 * fury_decode_host_execute below). */
int fury_row_decode_host(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                         int64_t nrows, fury_column* columns, int32_t device);

/* Host-memory decode of ANY schema (nested beans, maps, lists of structs / strings, collection
 * schemas), in the two steps of the device API (the output sizes depend on the data):
 * fury_decode_host_prepare stages the rows in HBM and returns every schema node's Arrow entries
 * and payload bytes (breadth-first node order, see fury_decode_prepare); the caller allocates the
 * host buffers from them (validity (entries + 7) / 8 bytes, offsets entries + 1 int32, values
 * entries * width / (entries + 7) / 8 for BOOL / node_bytes for STRING-BINARY (checked against
 * fury_column.capacity) / 16 * entries for DECIMAL) and calls fury_decode_host_execute, which
 * decodes in HBM and copies every buffer back (synchronous; with tuning "host_decode_inplace" the
 * values / offsets / payloads of pinned outputs are written in place -- slower).
 * The plan is freed by
 * fury_decode_plan_destroy.  Replaces generated fromRow + ArrowWriter for nested beans
 * (FMT/encoder/BaseBinaryEncoderBuilder.java:459-706, FMT/vectorized/ArrowWriter.java:519-640). */
int fury_decode_host_prepare(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                             int64_t nrows, int64_t* node_entries, int64_t* node_bytes,
                             fury_decode_plan** plan, int32_t device);
int fury_decode_host_execute(fury_decode_plan* plan, fury_column* columns);

/* ---- JNI core (java/.../GpuRowEncoder.java's native methods, minus the JNIEnv marshalling) ---
 * The exact arrays GpuRowEncoder builds, decoded in this library (fury_row_jni.cc only copies Java
 * arrays in and out and throws fury_jni_exception_class(status)).  Reference surface:
 * Encoders.bean(...) / RowEncoder (FMT/encoder/Encoders.java:60-219, RowEncoder.java:26-32).
 *   names / meta: flattenField in pre-order -- names[i] and meta[3 i .. 3 i + 2] = {typeId,
 *     nullable, numChildren} of node i (a MAP's children are key and value; `nodes` entries, the
 *     first `top` subtrees are the bean's fields in slot order);
 *   desc: describe() in pre-order -- 5 int64 per schema node {values address, validity address,
 *     offsets address, values capacity, numChildren} (host addresses); its child counts must
 *     match the schema's (FURY_ERR_INVALID_ARGUMENT otherwise);
 *   counts: 2 int64 per node (breadth-first, fury_decode_prepare order): entries, payload bytes;
 *   counts_len (the Java array's length) below 2 * fury_schema_num_nodes is
 *   FURY_ERR_INVALID_ARGUMENT, nothing written. */
const char* fury_jni_exception_class(int status);   /* Java class name of a status, NULL for OK */
int fury_jni_schema_create(const char* const* names, const int32_t* meta, int32_t nodes,
                           int32_t top, fury_schema** out);
int fury_jni_encode_host(const fury_schema* schema, const int64_t* desc, int64_t desc_len,
                         int64_t nrows, void* rows, int64_t rows_capacity, int64_t* row_offsets,
                         int64_t* row_bytes, int32_t device);
int fury_jni_decode_host(const fury_schema* schema, const void* rows, const int64_t* row_offsets,
                         int64_t nrows, const int64_t* desc, int64_t desc_len, int32_t device);
int fury_jni_decode_host_prepare(const fury_schema* schema, const void* rows,
                                 const int64_t* row_offsets, int64_t nrows, int64_t* counts,
                                 int64_t counts_len, fury_decode_plan** plan, int32_t device);
int fury_jni_decode_host_execute(const fury_schema* schema, fury_decode_plan* plan,
                                 const int64_t* desc, int64_t desc_len);

/* ---- Arrow IPC (ArrowUtils.serializeRecordBatch, FMT/vectorized/ArrowUtils.java:63-72;
 *      ArrowSerializers stream writers, FMT/vectorized/ArrowSerializers.java:128-167) --------- */
/* Encapsulated IPC Schema message of the schema, in HOST memory:
 * [0xFFFFFFFF][int32 metadata size][flatbuffer Message<Schema>][padding to 8].  *len receives
 * the size; out == NULL only sets *len, a too small cap returns FURY_ERR_CAPACITY.  An IPC
 * stream is this message, then record batch messages, then the 8-byte end-of-stream marker
 * [0xFFFFFFFF][0x00000000] (ArrowStreamWriter.writeEndOfStream). */
int fury_arrow_ipc_schema(const fury_schema* schema, uint8_t* out, int64_t cap, int64_t* len);
/* Encapsulated IPC RecordBatch message of device columns (fury_rows_to_arrow output, or any
 * columns in that layout) written to DEVICE memory `out` (16-byte aligned): flatbuffer metadata,
 * then the body = every Arrow buffer in pre-order (validity, offsets, values; children after
 * their parent; a MAP's "entries" struct node in between), each padded to 64 bytes.  Null
 * counts are computed on the device from the validity bitmaps.  The lengths of variable-size
 * buffers are read back from the device offsets, so the call is synchronous on `stream`.
 * out == NULL only sets *len. */
int fury_arrow_ipc_record_batch(const fury_schema* schema, const fury_column* columns,
                                int64_t nrows, void* out, int64_t cap, int64_t* len, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FURY_ROW_H_ */
