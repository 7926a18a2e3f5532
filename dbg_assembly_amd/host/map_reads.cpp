// map_reads -- the link_scaffold module's single-read mapper (link_scaffold/map_reads.cpp) with every read mapped on the
// GPU (MAP section of include/dbgk.h).  Same command line, same output files: per reads file <name>.map_reads.2ctg.gz,
// .2ctg.gz.reads.fa.gz, .1ctg.gz and .stat in -o, and <lib>.map_reads.2ctg.lib beside the library file, identical to the
// reference's after decompression.  -t sizes nothing on the device.
#include <ctime>

#include "map_common.h"

static int threadNum = 10;
static const char *const ReadIdDelims = ">@ \t\n"; // make_read_id of map_reads.cpp:312

static void usage()
{
	cout << "\nFunction instruction:"
	        "\n\nmap_reads, maps single illumina reads onto the contig sequences, using similar alignment method with map_pair. "
	        "One read could at most be mapped to two contigs, and only those reads mapped to two different contigs could be used "
	        "to link contigs and fill the gaps between contigs. Tt is recommended to set parameter MinCtgLen (-l) to be 1/2 * MinReadLen (-r). "
	        "The output of map_reads is the input of link_scafftig. \n";
	cout << "\nmap_reads  <contig_file.fa>  <reads_files.lib>\n"
	     << "   Function:  map single reads onto contigs" << endl
	     << "   Version: 1.0" << endl
	     << "   -k <int>     kmer size (construct hash), default=" << KmerSize << endl
	     << "   -s <int>     seed size (number of contained kmers in a seed), default=" << SeedKmerNum << endl
	     << "   -l <int>     contigs not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinCtgLen << endl
	     << "   -r <int>     reads not shorter than this cutoff are used for mapping [and scaffolding], default=" << MinReadLen << endl
	     << "   -i <float>   minimum mapping identity, default=" << MinMapIdentity << endl
	     << "   -f <int>     input file format: 1: fq|gz(one-line), 2: fa|gz(one-line), default=" << Input_file_format << endl
	     << "   -o <str>     output direcotry, default = " << Output_prefix << endl
	     << "   -t <int>     number of threads to run in parallel, default=" << threadNum << endl
	     << "   -h           get the help information\n" << endl
	     << "Example: map_reads  -l 125 -r 250 -t 10 -o ./maping_results/  Ecoli.contig.fa illumina_reads.lib" << endl
	     << endl;
	exit(0);
}

// the counters of one reads file and the text of a batch on its way to the three output files
struct ReadsTally {
	uint64_t total_read_num = 0, map_ctg_diff_num = 0, map_ctg_same_num = 0, map_no_no_num = 0, error_map_num = 0;
	void write(ofstream &MapCtgStat) const
	{
		MapCtgStat << "\ttotal_read_num: " << total_read_num << endl;
		MapCtgStat << "\tmap_ctg_diff_num: " << map_ctg_diff_num << "  " << (double)map_ctg_diff_num / total_read_num * 100 << "%" << endl;
		MapCtgStat << "\tmap_ctg_same_num: " << map_ctg_same_num << "  " << (double)map_ctg_same_num / total_read_num * 100 << "%" << endl;
		MapCtgStat << "\tmap_no_no_num: " << map_no_no_num << "  " << (double)map_no_no_num / total_read_num * 100 << "%" << endl;
		MapCtgStat << "\terror_map_num: " << error_map_num << "  " << (double)error_map_num / total_read_num * 100 << "%" << endl;
	}
};

// the reads of a batch with their hits -> the lines of the three files (the loop of map_reads.cpp:330-390)
static void rows_of_batch(const Contigs &ctg, const vector<string> &ids, const char *bases, const uint64_t *offsets, const dbgk_map_hit *hits, size_t n,
                          ReadsTally &T, ostringstream &diff, ostringstream &seq, ostringstream &same)
{
	for (size_t i = 0; i < n; i++) {
		const size_t len = offsets[i + 1] - offsets[i];
		if (len < (size_t)MinReadLen) continue;
		T.total_read_num++;
		const dbgk_map_hit &a = hits[2 * i], &b = hits[2 * i + 1];
		if (a.contig != -1) {
			if (b.contig != -1) {
				if (a.contig != b.contig) {
					T.map_ctg_diff_num++;
					ctg.row(diff, ids[i], len, a);
					diff << "\t";
					ctg.row(diff, ids[i], len, b);
					diff << "\n";
					seq << ">" << ids[i] << "\n";
					seq.write(bases + offsets[i], len);
					seq << "\n";
				} else {
					T.error_map_num++;
				}
			} else {
				T.map_ctg_same_num++;
				ctg.row(same, ids[i], len, a);
				same << "\n";
			}
		} else {
			T.map_no_no_num++;
		}
	}
}

// one reads file (parse_one_reads_file, map_reads.cpp:198-403)
static void parse_one_reads_file(const Contigs &ctg, const string &reads_file)
{
	const string name = Output_prefix + "/" + base_name(reads_file);
	GzWriter MapCtgDiff(name + ".map_reads.2ctg.gz"), MapCtgDiffSeq(name + ".map_reads.2ctg.gz.reads.fa.gz"), MapCtgSame(name + ".map_reads.1ctg.gz");
	const string stat_file = name + ".map_reads.stat";
	ofstream MapCtgStat(stat_file.c_str());
	if (!MapCtgStat) cerr << "fail to open output file " << stat_file << endl;
	MapCtgDiff.write(string(HeaderOne) + HeaderTwo + "\n");
	MapCtgSame.write(string(HeaderOne) + "\n");

	ReadsTally T;
	LineReader in(reads_file);
	ReadBatch batch;
	vector<string> ids;
	const char mark = Input_file_format == 1 ? '@' : '>';

	auto flush = [&]() {
		batch.map(ctg.mapper);
		ostringstream diff, seq, same;
		rows_of_batch(ctg, ids, batch.bases.data(), batch.offsets.data(), batch.hits.data(), batch.size(), T, diff, seq, same);
		MapCtgDiff.write(diff.str());
		MapCtgDiffSeq.write(seq.str());
		MapCtgSame.write(same.str());
		batch.clear();
		ids.clear();
	};

	// the record loop of map_reads.cpp:295-320: a header line, the read, and for fastq two more lines
	string head, read, unused;
	while (in.getline(head)) {
		if (head.empty() || head[0] != mark) continue;
		in.getline(read);
		if (Input_file_format == 1) {
			in.getline(unused);
			in.getline(unused);
		}
		ids.push_back(make_read_id(head, ReadIdDelims));
		batch.add(read);
		if (batch.full()) flush();
	}
	flush();
	MapCtgDiff.close();
	MapCtgDiffSeq.close();
	MapCtgSame.close();
	T.write(MapCtgStat);
}

// DBGK_TEXT=device: parse_one_reads_file on the route where the text of the file never becomes strings.  Window by window
// (ParsedFile of map_common.h): the parser's batch -> dbgk_map_reads_device_keep, the hits left on the device -> dbgk_maprow_take_hits
// -> dbgk_maprow_rows_device, which classifies the reads and composes the lines of the three files -> GzWriter::write_device per
// stream.  The loop above and the parser ignore the same lines, so nothing is refused.  The files, the .stat file and stderr are
// byte for byte those of the loop above.  A batch with a row the device cannot print (dbgk_maprow_info.unprintable) goes through
// rows_of_batch instead.
static void parse_one_reads_file_on_device(const Contigs &ctg, const string &reads_file)
{
	const string name = Output_prefix + "/" + base_name(reads_file);
	GzWriter MapCtgDiff(name + ".map_reads.2ctg.gz"), MapCtgDiffSeq(name + ".map_reads.2ctg.gz.reads.fa.gz"), MapCtgSame(name + ".map_reads.1ctg.gz");
	GzWriter *const out[DBGK_MAPROW_STREAMS] = {&MapCtgDiff, &MapCtgSame, &MapCtgDiffSeq};
	const string stat_file = name + ".map_reads.stat";
	ofstream MapCtgStat(stat_file.c_str());
	if (!MapCtgStat) cerr << "fail to open output file " << stat_file << endl;
	MapCtgDiff.write(string(HeaderOne) + HeaderTwo + "\n");
	MapCtgSame.write(string(HeaderOne) + "\n");

	ReadsTally T;
	ParsedFile in(reads_file);
	uint64_t records = 0, out_bytes = 0, host_batches = 0;
	double ms_map = 0, ms_rows = 0;
	while (in.next()) {
		const uint64_t n = in.pi.n_records;
		if (n) {
			records += n;
			in.map_into(ctg, 0, n);
			dbgk_map_stats ms;
			int rc = dbgk_map_batch_stats(ctg.mapper, &ms);
			if (rc) die("dbgk_map_batch_stats", rc);
			ms_map += ms.ms_map + ms.ms_long;
			dbgk_maprow_info ri;
			rc = dbgk_maprow_rows_device(ctg.rows, &in.side, n, &ri);
			if (rc) die("dbgk_maprow_rows_device", rc);
			ms_rows += ri.ms_scan + ri.ms_write;
			if (ri.unprintable || rows_forced_to_host()) {
				vector<string> heads, ids(n);
				string bases;
				vector<uint64_t> offsets;
				vector<dbgk_map_hit> hits;
				in.to_host(ctg, n, heads, bases, offsets, hits);
				for (uint64_t i = 0; i < n; i++) ids[i] = make_read_id(heads[i], ReadIdDelims);
				ostringstream diff, seq, same;
				rows_of_batch(ctg, ids, bases.data(), offsets.data(), hits.data(), n, T, diff, seq, same);
				MapCtgDiff.write(diff.str());
				MapCtgDiffSeq.write(seq.str());
				MapCtgSame.write(same.str());
				host_batches++;
			} else {
				T.total_read_num += ri.counters[0], T.map_ctg_diff_num += ri.counters[1], T.map_ctg_same_num += ri.counters[2];
				T.map_no_no_num += ri.counters[3], T.error_map_num += ri.counters[4];
				for (int s = 0; s < DBGK_MAPROW_STREAMS; s++) {
					out[s]->write_device(ctg.rows, s);
					out_bytes += ri.stream_bytes[s];
				}
			}
		}
		in.in.keep_from(in.pi.consumed);
	}
	MapCtgDiff.close();
	MapCtgDiffSeq.close();
	MapCtgSame.close();
	if (getenv("DBGK_TIMINGS"))
		cerr << "Text on device: " << in.in.windows << " windows, " << records << " records, " << out_bytes << " bytes of rows, " << host_batches
		     << " batches through the host loop; device ms: parse " << in.ms_parse << ", map " << ms_map << ", rows " << ms_rows << endl;
	T.write(MapCtgStat);
}

int main(int argc, char *argv[])
{
	int c;
	while ((c = getopt(argc, argv, "k:s:l:r:i:f:o:t:h")) != -1) {
		switch (c) {
			case 'k': KmerSize = atoi(optarg); break;
			case 's': SeedKmerNum = atoi(optarg); break;
			case 'l': MinCtgLen = atoi(optarg); break;
			case 'r': MinReadLen = atoi(optarg); break;
			case 'i': MinMapIdentity = atof(optarg); break;
			case 'f': Input_file_format = atoi(optarg); break;
			case 'o': Output_prefix = optarg; break;
			case 't': threadNum = atoi(optarg); break;
			case 'h': usage(); break;
			default: usage();
		}
	}
	if (argc < 3 || argc - optind < 2) usage();
	const string contig_seq_file = argv[optind++];
	const string reads_lib_file = argv[optind++];

	const clock_t time_start = clock();
	cerr << "\nProgram start ............" << endl;
	vector<string> reads_files;
	reading_lib_file(reads_lib_file, reads_files);
	cerr << "\nInput reads file number: " << reads_files.size() << endl;
	for (const string &f : reads_files) cerr << f << endl;

	{
		const string mapped_2ctg_file = reads_lib_file + ".map_reads.2ctg.lib";
		ofstream TwoCtgFile(mapped_2ctg_file.c_str());
		for (const string &f : reads_files) TwoCtgFile << Output_prefix << "/" << f << ".map_reads.2ctg.gz" << endl;
	}

	Contigs ctg;
	ctg.load(contig_seq_file, 1);
	const bool on_device = text_on_device();
	if (on_device) ctg.rows_on_device(DBGK_MAPROW_READS, ReadIdDelims);
	make_output_dir();

	cerr << "\nAlign input reads to the kmer-hash: " << endl;
	for (const string &f : reads_files) {
		cerr << "\n\tParse " << f << " ............." << endl;
		if (on_device) parse_one_reads_file_on_device(ctg, f);
		else parse_one_reads_file(ctg, f);
	}
	cerr << "\nProgram finished !" << endl;
	cerr << "Run time: " << double(clock() - time_start) / CLOCKS_PER_SEC << endl;
	return 0;
}
